// swb_kernels.hip.inc -- device code of the batched Spriteworld step/render engine (gfx950).
//
// A step is two kernels on one stream:
//
//   "cover"     one 64-lane wavefront owns one environment (64-thread workgroups: no barriers, no inter-wave
//               communication) and runs, in order:
//     P0  state   : auto-reset from the pool, action apply (hit-test with lanes = polygon edges),
//                   velocity update + clip, task reward / success spread over the lanes (lanes =
//                   sprites / clusters, sums in numpy's order), termination   (FP64)
//     P1  geometry: lanes = the vertices / edges of ALL sprites, 64 per pass: centred paths (FP64, no
//                   FMA) -> canvas ints -> Pillow add_edge + "connect discontiguous corners" pre-pass
//     P2  coverage: per batch of 64 rows of the anti-aliased canvas (starting at the next row some
//                   sprite covers), sprites front-to-back: float32 scan-line crossings -> per-row bit
//                   masks (parity toggles + crossing pixels) -> visible spans (occlusion by bit ops)
//                   -> RUNS of identical canvas rows, appended to a list in HBM (a few hundred bytes to
//                   ~2 KB per environment) per group of 64 output columns.  (Canvases wider than 320 px, where a sprite
//                   spans several batches: only the edges with rows in the batch share the lanes, and the x-chunks of a
//                   wide sprite hand the parity on -- coverage_batch2.)
//   "resample"  one wavefront per (environment, group of 64 output columns, band of output rows), needing
//               nothing but the run list, 16 colours and the filter tables (8 waves per SIMD):
//     P3  resample: lanes = output columns; per run the horizontal LANCZOS pass is a sum over the visible
//                   spans of colour * (prefix-summed fixed-point weights), exact; its uint8 result feeds
//                   the vertical pass kept as <= 8 in-flight accumulators per lane in registers (no
//                   canvas, no intermediate image)
//     P4  store   : finished output rows are packed in registers and written flipped, coalesced.
//   (anti_aliasing = 1: "fill" instead of "resample" -- the canvas is the image.)
//
// Why two kernels: the phases want different machines.  P0..P2 are latency-bound, need LDS and ~100 vector
// registers; P3 is pure vector-ALU work over a list that a scalar unit streams, and a wave of it that carries
// nothing of P0..P2 fits in 64 registers.  Fused (rounds 1-2: 128 registers, 4 waves per SIMD, one wave per
// environment for 45-125 us) a launch of 8192 environments was two rounds of waves followed by an 85 us drain in
// which the SIMDs ran 1-3 waves (profiles/r03_wave_timeline.md).
//
// Arithmetic follows oracle/sw_oracle.c operation for operation (which is pinned against the
// unmodified reference); reference citations are on each device function.
#ifndef SWB_SETS_PASS       // (the second pass of this file over itself compiles two kernel bodies only: see swb_cover_kernel)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/swb.h"

#define SWB_WAVE 64
#ifndef SWB_WORD_GROUPS
#define SWB_WORD_GROUPS 4     // P2: canvas words outside a sprite's chunk are skipped this many at a time (NW > 5)
#endif
#ifndef SWB_AES_MIN_ITERS
#define SWB_AES_MIN_ITERS 4   // P2: the "active edges" lane mapping is tried where the plain ones need this many iterations
#endif
#ifndef SWB_AES_MAX_NARROW_NW
#define SWB_AES_MAX_NARROW_NW 10   // ... and only in the cover kernels of canvases wider than this many 32-px words
#endif
#ifndef SWB_COVER_WAVES_PER_SIMD
#define SWB_COVER_WAVES_PER_SIMD 5        // register budget of the cover kernel on canvases up to 320 px wide: 96 VGPRs, no spills
#endif
#ifndef SWB_COVER_WAVES_PER_SIMD_NARROW
#define SWB_COVER_WAVES_PER_SIMD_NARROW 6 // ... on canvases up to 64 px wide (anti_aliasing = 1 above all): 80 VGPRs, four spilled registers, but
#endif                                    // their LDS footprint (6 KB) lets the sixth wave in: 8192 waves on 6144 slots, -6 % (measured)
#ifndef SWB_COVER_WAVES_PER_SIMD_WIDE
#define SWB_COVER_WAVES_PER_SIMD_WIDE 4   // ... on wider canvases (covered[] = 20 registers)
#endif
#ifndef SWB_RS_WAVES_PER_SIMD
#define SWB_RS_WAVES_PER_SIMD 8           // resample / fill kernels: 64 VGPRs
#endif
#define SWB_COVER_WAVES(NW) ((NW) <= 2 ? SWB_COVER_WAVES_PER_SIMD_NARROW : ((NW) <= 10 ? SWB_COVER_WAVES_PER_SIMD : SWB_COVER_WAVES_PER_SIMD_WIDE))
#define SWB_RS_WAVES_PER_BLOCK 4          // ... in workgroups of 4 waves that share the horizontal prefix table in LDS
#define SWB_VSLOTS 8          // in-flight output rows of the vertical pass
// Sprites per environment the tuned kernels (cover, resample, fill) are built for: their LDS, prefix scans and task scratch
// are sized by it.  Handles of more sprites (up to SWB_MAX_SPRITES) run swb_ms_state_kernel and the large-frame kernels.
#define SWB_TUNED_SPRITES 16
#define PRECISION_BITS 22

// One environment's last task evaluation (swb_params::task_cache): 16 bytes, read and written as one uint4.
struct swb_task_record {
  uint32_t tr_lo, tr_hi;       // the task reward, float64 bits
  uint8_t ok, err;             // task.success; the swb_env_error bits the evaluation raised
  uint16_t pad_;
  uint32_t stamp;              // swb_params::task_epoch of the launch that wrote it (0: never written)
};
static_assert(sizeof(swb_task_record) == 16, "a task record is one 16-byte load");

struct swb_params {
  // ---- config
  int32_t N, S, AA;
  int32_t Wo, Ho;           // PIL output (width, height) = (image_size[0], image_size[1])
  int32_t Wc, Hc;           // canvas
  uint32_t bg;              // r | g<<8 | b<<16
  int32_t action_space, keep_in_frame, max_episode_length, pos_is_f32, action_is_f32;
  double action_scale, motion_cost;
  int32_t n_tasks, is_meta, meta_aggregator, meta_termination;
  double meta_terminate_bonus;
  swb_task tasks[SWB_MAX_TASKS];
  // ---- constant tables
  const double* shape_verts;   // [total][2]
  const int32_t* shape_off;    // [SWB_MAX_SHAPES + 1] (n_shapes + 1 offsets, padded with the last one)
  int32_t max_verts;           // max vertices of any shape
  const double* shape_dmin;    // [SWB_MAX_SHAPES] (padded with zeros) smallest distance between two vertices of the shape (unit scale)
  const int32_t* h_xmin;       // [Wo]
  const int32_t* h_cnt;        // [Wo]
  const int32_t* h_tbl;        // [Wo] offset of the column's prefix vector in h_pfx
  const int32_t* h_pfx;        // [h_pfx_len] unique prefix-sum vectors
  int32_t h_pfx_len;
  const int32_t* v_tab;        // [Hc][SWB_VSLOTS] coefficient of canvas row y for accumulator slot j = out_row % VS
  const int32_t* v_pfx;        // [Hc + 1][SWB_VSLOTS] prefix sums of v_tab over canvas rows (runs of identical rows)
  const int32_t* v_end;        // [Ho + 2] last canvas row contributing to output row r (padded with two huge entries)
  // ---- pool
  const int32_t* p_n;
  const double *p_x, *p_y, *p_xv, *p_yv, *p_scale, *p_ca, *p_sa;
  const int32_t* p_shape;
  const uint32_t* p_rgb;       // [P][S] packed r|g<<8|b<<16
  const int8_t* p_label;       // [P][T][S]
  const int8_t* p_cell_label;  // [P][T][S][SWB_MAX_CELLS] labels per cell of the position grid of the tasks that key on position
                               // (swb_task::n_xcuts / n_ycuts); NULL when no task does
  const int32_t *pool_base, *pool_len;
  const double *p_angle, *p_color;   // [P][S], [P][S][3] (SpriteFactors observation only)
  // ---- live state
  double *x, *y;               // [N][S]
  int32_t *nspr, *entry, *step_count, *episode;
  uint8_t* reset_next;
  // ---- per-step io
  const void* actions;
  uint8_t* obs;
  double* reward;
  float* discount;
  uint8_t *step_type, *success, *error;
  int32_t render_only;         // 1: observation() only, no state change; 2: success() only -- the task evaluated on the sprites
                               // as they are (after setters / swb_set_positions), nothing else written (obs is NULL)
  int32_t lds_per_wave;        // bytes
  int32_t outrow_bytes;        // size of wave_lds::outrow
  int32_t max_edges;           // S * max_verts
  int32_t cpath_in_masks;      // centred paths fit in the (idle) mask arrays during P0/P1
  int32_t max_spans;           // M: visible spans per canvas row the LDS lists are sized for
  int32_t span_cap;            // ... and how many of them are used (= M; tests lower it to force the HBM slots)
  uint32_t* ovf;               // [ovf_slots][64][ovf_cap] spans beyond the register + LDS lists: one slot per wave that
                               // ever needs it (virtually none), taken from a bitmap and given back at kernel end
  uint32_t* ovf_bitmap;        // [ovf_slots / 32] slots in use
  int32_t ovf_slots;           // a multiple of 32, >= the waves that can be resident at once
  int32_t ovf_cap;             // overflow spans per canvas row (min(Wc/2 + 1, 32)); a row beyond 3 + M + ovf_cap
                               // visible spans sets SWB_ENV_ERR_SPAN_OVERFLOW
  // ---- hand-off from the cover kernel (P0..P2) to the resample / fill kernel (P3, P4): per environment and per
  // group of 64 output columns a list of RUNS of identical canvas rows with their visible spans, in 8-byte units
  //   unit 0: { row | (rows - 1) << 16 | continuation << 23 | spans << 24,  span 0 }      span = start | end << 10 | sprite << 20
  //   unit 1: { span 1, span 2 }   (when spans >= 2; an absent span is 0 = empty)
  //   unit k: { span 2k-1, span 2k }   (spans > 3)
  // A CONTINUATION run (SWB_RUN_CONTINUES, anti_aliasing > 1 only) is unit 0 alone: its rows have the spans of the run before it in
  // the list, the spans field repeats that run's count (at least 1), span 0 is not read.  Bit 22 is free.
  // and a header (SWB_RHDR_DWORDS dwords): [0,16) colour minus background of sprite s as three signed 10-bit fields,
  // [16,32) its colour r | g << 8 | b << 16, then per column group { units in the list, first unit of band b ... }
  uint32_t* runs;              // [N][ncg][2 * run_cap]
  uint32_t* rhdr;              // [N][SWB_RHDR_DWORDS]
  int32_t run_cap;             // units of a list's own part.  A list that outgrows it MOVES to a segment of the shared arena below,
                               // twice (four times ...) as large -- the wave copies what it has written so far -- so that a list stays
                               // one contiguous array wherever it lives and the second kernel's loop knows nothing of it: every
                               // position in the header (band starts, list end) is counted from the first unit of the list's OWN
                               // part, a list in the arena simply has positions beyond run_cap.  A scene that finds the arena
                               // exhausted sets SWB_ENV_ERR_SPAN_OVERFLOW
  uint32_t* arena_head;        // [2] units taken from the arena by the launch of parity 0 / 1 (a launch's first block zeroes
                               // the OTHER word: the next launch starts after this one has ended); segments are multiples of 32 units
  int64_t arena_base;          // first unit of the arena, in units from `runs` (= N * ncg * run_cap)
  int32_t arena_units;         // its capacity; 0: none (a list ends with its own part)
  int32_t arena_pad_;
  int32_t ncg;                 // groups of 64 output columns (ceil(Wo / 64))
  int32_t nbands;              // bands of output rows: one (environment, column group, band) per wave of the resample kernel
  const int32_t* band_lo;      // [nbands + 1] first output row of band b (band b = rows [band_lo[b], band_lo[b + 1]))
  const int32_t* band_y0;      // [nbands] first canvas row that feeds the band's first output row
  const int32_t* band_first;   // [nbands] oldest output row still in flight at that canvas row; band_lo is chosen so that
                               // band_first % VS == 0 (the band's first in-flight row accumulates in slot 0)
  const uint32_t* v_break;     // [2][ceil(Hc / 32) + 3] bit y of table 0 set: canvas row y starts a new run (an output row ended on y - 1, or a band starts at y); of table 1: a band starts at y
  const int32_t* cg_lo;        // [ncg] canvas columns [cg_lo, cg_hi) are the ones a column group's resampling windows reach
  const int32_t* cg_hi;
  // ---- cost-ordered dispatch: the cover kernel files every environment under the length of its run list (a good
  // measure of the resample work it causes, and of the next step's cover work: a scene changes little from step
  // to step); the resample kernel then takes the environments longest first, dealt over the SIMDs like cards.
  // (Steering the NEXT cover launch with the same lists -- longest first, so that its second round of waves holds
  // the light scenes -- was measured too: -5 % on 12-sprite scenes, +2 % on the headline; not kept.)
  // Filing is one returning atomic per environment: the counters are sharded by environment % 8 (8 x 32 words), else
  // 8192 waves queue on the ten or so buckets in use (measured: +50 us per launch).  Block b of either kernel serves
  // shard b % 8 -- observed to be the XCD the environment's cover block ran on, so the lists are read from its L2.
  uint32_t* cost_cnt;          // entries per bucket, [SWB_COST_SHARDS][SWB_COST_BUCKETS] per set: two sets of kind 0 (tasks of the
                               // resample / fill kernel: this launch's and the next one's), three sets of kind 1 (environments for
                               // the next cover launch, see cover_order: the previous launch's, this one's, the next one's), then
                               // the SWB_COST_WORD_* words
  int32_t* cost_list;          // [2][SWB_COST_SHARDS][SWB_COST_BUCKETS][cost_cap] the tasks of each bucket, in arrival order:
                               // environment | column group << 24, each under the length of its own list
  int32_t cost_cap;            // ncg * ceil(N / SWB_COST_SHARDS)
  int32_t cost_range0;         // the cost range the buckets of kind 0 span until a launch has measured one (SWB_COST_WORD_KEY_*)
  int32_t parity;              // set of this launch (0 / 1)
  int32_t deal_shift;          // log2 of the compute units per XCD (dealt_block), 0: plain descending order
  // ---- cover launches in order of decreasing cost.  8192 waves on 5120 slots are 1.6 rounds: what an environment cost in the
  // previous step (wave cycles: 0.95 correlated from step to step) decides its place in this one -- the heavy scenes first, so
  // that the second round holds the light ones (list scheduling, longest first).  The cover wave files its environment under
  // its own cycle count (kind 1 of cost_cnt, lists in ccost_list); the next launch's block b takes entry b / 8 of shard b % 8.
  // The host sets cover_order only when the previous launch filed every environment.
  int32_t* ccost_list;         // [3][SWB_COST_SHARDS][SWB_COST_BUCKETS][ceil(N / SWB_COST_SHARDS)]
  int32_t cover_order;
  int32_t cphase;              // launch count % 3: the set of kind 1 this launch files into (it reads the one before, clears the one after)
  int32_t prio_div;            // a priority level = the mean work of a wave / prio_div, rounded down to a power of two
  int32_t prio_levels;         // bit 0: resample waves set their priority by the list they have left (see there); bit 1: cover waves
                               // by the cycles they are expected to have left
  int32_t paint_in_cover;      // 1: anti_aliasing = 1 and an image of up to 64 columns -- the cover kernel (its PAINT build) writes the frame itself
  int32_t band_tasks;          // 1: (small batches: nbands > 1) a task of the second kernel is an (environment, column group, BAND), filed under the
                               // cost of the band's own part of the list: entry = environment | column group << 24 | band << 26
  // ---- live sprite overrides (sprite.py:152-175 attribute setters, swb_set_sprite_attr).  Read only by the
  // OV = true kernels, which an engine launches once a setter has been called; an environment whose flag is
  // set takes shape / scale / labels / centred paths of its sprites from these arrays instead of the pool,
  // until its next reset clears the flag.  (Appended last: the other kernels' argument offsets do not move.)
  uint8_t* ov_flag;            // [N]; then, on a 64-byte line of its own (SWB_OV_SLOT), ONE device pointer: the task-set block
                               // of the handle (swb_set_task_sets; DESIGN.md section 31) -- SWB_SET_TABLE_BYTES of
                               // swb_task_set[SWB_MAX_TASK_SETS], then [P] the set of every pool entry -- or NULL.  It hangs
                               // here, behind memory only the OV kernels read, so that this block does not grow by a byte:
                               // the kernels of handles without task sets, their argument sizes and offsets stay what they were
  const int32_t* ov_shape;     // [N][S]
  const double* ov_scale;      // [N][S]
  const double* ov_angle;      // [N][S]  degrees (SpriteFactors observation)
  const int8_t* ov_label;      // [N][T][S]
  const double* ov_cpath;      // [N][S][SWB_MAX_SHAPE_VERTS][2] centred paths as the setters left them
  const int8_t* ov_cell_label; // [N][T][S][SWB_MAX_CELLS] (handles with tasks that key on position)
  // ---- kept run lists (the cover kernel, non-PAINT builds).  A list is a pure function of the environment's sprites and of the
  // handle's geometry, and the lists persist from launch to launch: a wave whose environment's header carries the stamp
  // `list_epoch` and whose sprites did not move in this launch files the list that is already there instead of building it
  // again.  The host bumps the epoch whenever something other than a step changes what a list depends on or where it lives.
  uint32_t list_epoch;         // 0: keep nothing and stamp the lists invalid (launches on a state view, SWB_NO_KEEP_LISTS)
  uint32_t list_pad_;
  unsigned long long* list_stats;   // [2] cover waves that kept / built their lists (SWB_LIST_STATS; else NULL)
  // ---- frame cache (swb_resample_kernel; DESIGN.md section 24).  A frame is a pure function of the run lists, the header's
  // colour words, the background and the resampling tables: where a cover wave KEPT its lists, the frame the resample waves
  // would compute is the one they computed at the previous launch.  The engine keeps its own copy of every environment's last
  // frame, laid out like `obs`; the header word SWB_RHDR_FRAME says what the resample waves of an environment do with it.
  // The caller's buffer is written in full at every launch all the same -- from the copy instead of from the lists.
  // The copies are made in the COVER launch, speculatively (spec_copy; DESIGN.md section 29): one more workgroup per
  // (environment, column group) copies the cached frame of every environment whose word is not 0, beside the waves that build.
  uint8_t* frame_cache;        // [N][Ho][Wo][3], NULL: the handle has none (every wave resamples)
  unsigned long long* frame_stats;  // [7] frames taken from the cache (counted as the tasks that copied them were) / resample tasks that
                                    // filled / resampled, then the wave cycles of the copies, of the others, the list bytes of the
                                    // others, and the copy workgroups that copied (SWB_LIST_STATS; else NULL)
  int32_t obs_aligned16;       // `obs` and every row segment of a column group start on 16 bytes: the copy moves 16 bytes per lane
  int32_t spec_copy;           // the cover grid holds N * ncg copy workgroups: 1 behind the N cover workgroups, 2 in front (SWB_SPEC_COPY); 0 none
  // ---- split bands (DESIGN.md section 26): lists and tables are built for nbands bands and band_tasks is on, but an environment
  // files its nbands band tasks only when it resamples or fills AND the launch's decision word (SWB_COST_WORD_SPLIT) says split;
  // otherwise -- and always when its frame is copied -- it files ONE task per column group with SWB_TASK_WHOLE set, which takes
  // the frame's whole rows and the whole list.  The word is written by the previous launch's cost_housekeeping: split when that
  // launch had at most split_when frames that resampled or filled (counted by their cover waves, SWB_COST_WORD_SPLIT_CNT).
  int32_t split_bands;         // 1: the mode is on
  int32_t split_when;
  int32_t split_carry;         // 1: this launch does not draw the live state (a state view): the next launch's word is this one's
  int32_t split_pad_;
  unsigned long long* split_stats;  // [3] resample tasks: whole ones that resampled / filled, band tasks, whole copies (SWB_LIST_STATS)
  // ---- active mask (swb_step_masked; DESIGN.md section 27).  An environment whose byte is 0 takes no part in the step: the state
  // phase leaves its state arrays and its entries of the outputs alone (a pending reset stays pending, its action row is not
  // read, no task is evaluated), and its frame is drawn from the state as it is -- on the two-kernel path its wave keeps its
  // lists like any wave whose sprites did not move.  Read once per wave, in load_env_state.  (Appended last, as above.)
  const uint8_t* active;       // [N], NULL: every environment takes part (and everything but a step: renders, evaluations, rollouts)
  // ---- task cache (finish_step; DESIGN.md section 28).  The task's reward, success and error bits are a pure function of the
  // sprites' positions, the episode's labels, the sprite count and the task block above: a step that is no reset and moved no
  // sprite bitwise takes them from the record the environment's last evaluation left, if that record carries `task_epoch`.  The
  // host bumps the epoch whenever something other than a step changes what the task depends on.  Bound only for launches that
  // step the live state (render_only == 0, no state view); the rollout kernels compile the cache out.  (Appended last, as above.)
  swb_task_record* task_cache; // [N], NULL: the handle has none (SWB_NO_TASK_CACHE), or the launch is no step: every wave evaluates
  uint32_t task_epoch;         // never 0: a zeroed record is stale
  uint32_t task_pad_;
  unsigned long long* task_stats;   // [2] stepping waves that reused / evaluated the task (SWB_LIST_STATS; else NULL)
};

#define SWB_SET_TABLE_BYTES ((int)(SWB_MAX_TASK_SETS * sizeof(swb_task_set)))    // the table in front of the entries' bytes
#define SWB_OV_SLOT(N) (((size_t)(N) + 63) & ~(size_t)63)                        // offset of the block's pointer behind ov_flag[N]
#define SWB_OV_FLAG_BYTES(N) (SWB_OV_SLOT(N) + 64)
// The task of one environment's episode, all wave-uniform: sub-tasks tasks[first() .. first() + n()) -- rows first() .. of the
// labels, too --, how they are aggregated, and when the episode times out.  SETS = false: the handle's one task, every member
// read from the config block where it is used -- the code of the kernels that know no task sets is the code they had before
// there were any.  SETS = true (task_view_of): the set the episode's pool entry names, or the config block where the block's pointer is NULL.
template <bool SETS> struct task_view;
template <> struct task_view<false> {
  const swb_params& p;
  __device__ __forceinline__ int first() const { return 0; }
  __device__ __forceinline__ int n() const { return p.n_tasks; }
  __device__ __forceinline__ int is_meta() const { return p.is_meta; }
  __device__ __forceinline__ int aggregator() const { return p.meta_aggregator; }
  __device__ __forceinline__ int termination() const { return p.meta_termination; }
  __device__ __forceinline__ int max_episode_length() const { return p.max_episode_length; }
  __device__ __forceinline__ double terminate_bonus() const { return p.meta_terminate_bonus; }
};
template <> struct task_view<true> {
  int first_, n_, is_meta_, aggregator_, termination_, max_episode_length_;
  double terminate_bonus_;
  __device__ __forceinline__ int first() const { return first_; }
  __device__ __forceinline__ int n() const { return n_; }
  __device__ __forceinline__ int is_meta() const { return is_meta_; }
  __device__ __forceinline__ int aggregator() const { return aggregator_; }
  __device__ __forceinline__ int termination() const { return termination_; }
  __device__ __forceinline__ int max_episode_length() const { return max_episode_length_; }
  __device__ __forceinline__ double terminate_bonus() const { return terminate_bonus_; }
};

// --------------------------------------------------------------------------------------------
// small helpers
// --------------------------------------------------------------------------------------------
// Read-only tables are read through the constant address space so that wave-uniform indices
// become scalar loads (s_load_*), not vector memory loads.
// THE RULE: only memory that NO wave of the same launch writes may go through as_const -- tables, the pool, and what an
// EARLIER kernel launch wrote (the resample / fill kernels read the run lists and headers of the cover kernel this way: a
// kernel boundary lies between writer and reader).  A load through the constant address space is "invariant" to the compiler:
// it may be hoisted above any fence or barrier, and the scalar cache is not coherent with stores of the same launch.  The
// round-3 team kernel (one workgroup per environment, lists handed from wave to wave behind a barrier) failed parity in exactly
// this way; memory written within the launch must be read with plain global loads.  Two places read same-launch words through
// plain loads on purpose: the dispatch counters (cost_cnt) and the overflow bitmap.
template <typename T>
using cptr = const T __attribute__((address_space(4)))*;
template <typename T>
__device__ __forceinline__ cptr<T> as_const(const T* q) { return (cptr<T>)(uintptr_t)q; }

__device__ __forceinline__ int lane_id() { return threadIdx.x & (SWB_WAVE - 1); }
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float rflf(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double rfld(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// Value of lane `src` (wave-uniform index) as a scalar: v_readlane, no LDS round trip.
__device__ __forceinline__ double readlane_d(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// Orders this wave's LDS traffic (hardware executes one wave's DS ops in order; this stops
// the compiler from moving or caching accesses across the point).  Never __syncthreads():
// waves of a block are independent environments and may have exited.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int wave_min_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// Pillow Draw.c ROUND_UP / ROUND_DOWN (float add for f >= 0, double for f < 0).
__device__ __forceinline__ int pil_round_up(float f) {
  if (f >= 0.0f) return (int)floorf(__fadd_rn(f, 0.5f));
  return (int)(-floor(__dadd_rn(fabs((double)f), 0.5)));
}
__device__ __forceinline__ int pil_round_down(float f) {
  if (f >= 0.0f) return (int)ceilf(__fsub_rn(f, 0.5f));
  return (int)(-ceil(__dsub_rn(fabs((double)f), 0.5)));
}
// Draw.c scan-line crossing: (y - y0) * dx + x0 in float32, no FMA.
__device__ __forceinline__ float pil_cross(int y, int y0, float dx, int x0) {
  return __fadd_rn(__fmul_rn((float)(y - y0), dx), (float)x0);
}

// sprite.py:96-101 + matplotlib affine_transform_2d: centred vertex i of a sprite (SURVEY A.3).
__device__ __forceinline__ void centered_vertex(const swb_params& p, int shape_o, int i, double scale,
                                                double ca, double sa, double& cx, double& cy) {
  const double vx = p.shape_verts[2 * (shape_o + i)], vy = p.shape_verts[2 * (shape_o + i) + 1];
  const double m00 = __dmul_rn(ca, scale), m01 = __dmul_rn(-sa, scale);
  const double m10 = __dmul_rn(sa, scale), m11 = __dmul_rn(ca, scale);
  cx = __dadd_rn(__dadd_rn(__dmul_rn(m00, vx), __dmul_rn(m01, vy)), 0.0);
  cy = __dadd_rn(__dadd_rn(__dmul_rn(m10, vx), __dmul_rn(m11, vy)), 0.0);
}

// sprite.py:113-115 -> matplotlib point_in_path (radius 0), even-odd rule (SURVEY A.4).
// Lanes = polygon edges of one sprite whose centred path (n vertices, float64 pairs) is in LDS;
// returns the wave-uniform containment of (tx, ty).
__device__ __forceinline__ bool contains_point_wave(const double2* cpath, int n, double tx, double ty) {
  const int l = lane_id();
  bool cross = false;
  if (l < n) {
    const double2 v0 = cpath[l], v1 = cpath[(l + 1 == n) ? 0 : l + 1];
    const bool f0 = (v0.y >= ty), f1 = (v1.y >= ty);
    if (f0 != f1) {
      const double lhs = __dmul_rn(__dsub_rn(v1.y, ty), __dsub_rn(v0.x, v1.x));
      const double rhs = __dmul_rn(__dsub_rn(v1.x, tx), __dsub_rn(v0.y, v1.y));
      cross = ((lhs >= rhs) == f1);
    }
  }
  return (__popcll(__ballot(cross)) & 1) != 0;
}

// sprite.py:103-107 Sprite.move under numpy in-place semantics (SURVEY A.2).
__device__ __forceinline__ double move1(int pos_f32, double pv, double motion, int keep) {
  double q = __dadd_rn(pv, motion);
  if (pos_f32) q = (double)(float)q;
  if (keep) {
    if (q < 0.0) q = 0.0;
    if (q > 1.0) q = 1.0;
  }
  return q;
}

// numpy pairwise sum (float64 / float32) of up to SWB_MAX_SPRITES (64) elements held in LDS; the code is numpy's for n <= 128.
__device__ __forceinline__ double np_sum_d(const double* a, int n) {
  if (n < 8) {
    double r = -0.0;
    for (int i = 0; i < n; ++i) r = __dadd_rn(r, a[i]);
    return r;
  }
  double r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = a[i];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __dadd_rn(r[j], a[i + j]);
  }
  double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                         __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __dadd_rn(res, a[i]);
  return res;
}
__device__ __forceinline__ float np_sum_f(const float* a, int n) {
  if (n < 8) {
    float r = -0.0f;
    for (int i = 0; i < n; ++i) r = __fadd_rn(r, a[i]);
    return r;
  }
  float r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = a[i];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], a[i + j]);
  }
  float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                        __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __fadd_rn(res, a[i]);
  return res;
}

// Length-2 float64 dot products in the orders the reference's numpy/BLAS calls use (pinned
// empirically, see oracle/sw_oracle.c norm2/dot2_hi/dot2_lo): einsum row norms have no FMA; the
// BLAS kernels accumulate with FMA, in an order that depends on the call shape.  With float32
// positions every product is exact in float64 and all orders agree.
__device__ __forceinline__ double norm2(double a0, double a1) {
  return __dadd_rn(__dmul_rn(a0, a0), __dmul_rn(a1, a1));
}
__device__ __forceinline__ double dot2_hi(double a0, double a1, double b0, double b1) {
  return __fma_rn(a1, b1, __dmul_rn(a0, b0));
}
__device__ __forceinline__ double dot2_lo(double a0, double a1, double b0, double b1) {
  return __fma_rn(a0, b0, __dmul_rn(a1, b1));
}

// tasks.py:127-128: np.float64 ** 0.5 is libm pow(x, 0.5); see swb_pow.hip.inc.
__device__ double swb_pow_half(double x);

// Scratch (per wave, LDS) for the task evaluation of up to NS sprites.  The tuned cover kernel's (task_scratch) aliases
// its span lists; the many-sprite state kernel has one of SWB_MAX_SPRITES entries.
template <int NS>
struct task_scratch_t {
  double xs[NS], ys[NS];
  double tmp[NS];
  double c0[NS], c1[NS], intra[NS];
  float tmpf[NS];
  double tr[SWB_MAX_TASKS];
  int tok[SWB_MAX_TASKS];
  int8_t lab[NS];
  double px0[NS];                                      // member distances grouped by cluster (Davies-Bouldin)
  int32_t cnt[NS];                                     // members per cluster
  uint32_t pres[4];                                    // labels present (bit set), 128 label values
  int8_t labels[SWB_MAX_TASKS * NS];                   // this episode's label[t][s], staged from the pool
};
typedef task_scratch_t<SWB_TUNED_SPRITES> task_scratch;

// the scratch aliases the LDS span lists: SWB_MIN_SPANS lists of 64 dwords must hold it
#define SWB_MIN_SPANS ((int)((sizeof(task_scratch) + 255) / 256))
static_assert(sizeof(task_scratch) <= 6 * 256, "task_scratch outgrew the span lists it aliases");

// --------------------------------------------------------------------------------------------
// Task evaluation (tasks.py): the reference's scalar arithmetic with the independent pieces spread
// over lanes -- lanes = sprites for the per-sprite distances (the libm
// pow, the square roots), lanes = clusters for centroids / intra-cluster means / the ratio matrix
// columns -- and every sum taken in numpy's order by one lane from LDS.  Lane s < n holds sprite
// s's position (px, py); results are wave-uniform.
// --------------------------------------------------------------------------------------------
// tasks.py:126-158 FindGoalPosition.
template <typename SC>
__device__ __forceinline__ void task_find_goal_wave(const swb_task& t, int n, double px, double py, const int8_t* label,
                                                    SC* sc, double* reward, int* success) {
  const int l = lane_id();
  const bool f = (l < n) && label[l < n ? l : 0] != 0;
  double r = 0.0;
  if (f) {
    const double d0 = __dsub_rn(px, t.goal_position[0]), d1 = __dsub_rn(py, t.goal_position[1]);
    const double w0 = __dmul_rn(t.weights_dimensions[0], __dmul_rn(d0, d0));
    const double w1 = __dmul_rn(t.weights_dimensions[1], __dmul_rn(d1, d1));
    const double dist = swb_pow_half(__dadd_rn(w0, w1));
    r = __dmul_rn(t.raw_reward_multiplier, __dsub_rn(t.terminate_distance, dist));
  }
  const unsigned long long fm = __ballot(f);
  const int m = __popcll(fm);
  const int all_ge0 = __ballot(f && !(r >= 0)) == 0ull;
  *success = all_ge0;
  if (m == 0) { *reward = __longlong_as_double(0x7ff8000000000000ll); return; }
  if (f) sc->tmp[__popcll(fm & ((1ull << l) - 1ull))] = r;
  wave_sync();
  const double dense = np_sum_d(sc->tmp, m);
  wave_sync();
  double rw = 0.0;
  if (all_ge0) { rw = __dadd_rn(rw, t.terminate_bonus); rw = __dadd_rn(rw, dense); }
  else if (!t.sparse_reward) { rw = __dadd_rn(rw, dense); }
  *reward = rw;
}

// scikit-learn 1.7.2 davies_bouldin_score (SURVEY A.8; oracle/sw_oracle.c davies_bouldin).
template <typename SC>
__device__ __forceinline__ int davies_bouldin_wave(int pos_f32, int n, double px, double py, const int8_t* label,
                                                   SC* sc, double* score_out) {
  const int l = lane_id();
  const int lab_l = (l < n) ? (int)label[l] : -1;
  const bool has = lab_l >= 0;
  const unsigned long long am = __ballot(has);
  const int m = __popcll(am);
  // labels present -> k, and the rank of each label among them (sklearn LabelEncoder)
  if (l < 4) sc->pres[l] = 0u;
  wave_sync();
  if (has) atomicOr(&sc->pres[lab_l >> 5], 1u << (lab_l & 31));
  wave_sync();
  const uint32_t q0 = sc->pres[0], q1 = sc->pres[1], q2 = sc->pres[2], q3 = sc->pres[3];
  const int k = __popc(q0) + __popc(q1) + __popc(q2) + __popc(q3);
  if (!(1 < k && k < m)) return SWB_ENV_ERR_DB_LABELS;
  if (has) {
    const int w = lab_l >> 5;
    const uint32_t qw = (w == 0) ? q0 : (w == 1) ? q1 : (w == 2) ? q2 : q3;
    const int rank = (w > 0 ? __popc(q0) : 0) + (w > 1 ? __popc(q1) : 0) + (w > 2 ? __popc(q2) : 0) +
                     __popc(qw & ((1u << (lab_l & 31)) - 1u));
    const int ci = __popcll(am & ((1ull << l) - 1ull));          // assigned sprites, order preserved
    sc->xs[ci] = px; sc->ys[ci] = py; sc->lab[ci] = (int8_t)rank;
  }
  wave_sync();
  // lanes = clusters: member count and centroid (sums in member order, in the position dtype)
  if (l < k) {
    int cnt = 0;
    double m0, m1;
    if (pos_f32) {
      float s0 = 0.f, s1 = 0.f;
      for (int i = 0; i < m; ++i)
        if (sc->lab[i] == l) {
          if (cnt == 0) { s0 = (float)sc->xs[i]; s1 = (float)sc->ys[i]; }
          else { s0 = __fadd_rn(s0, (float)sc->xs[i]); s1 = __fadd_rn(s1, (float)sc->ys[i]); }
          ++cnt;
        }
      m0 = (double)__fdiv_rn(s0, (float)cnt); m1 = (double)__fdiv_rn(s1, (float)cnt);
    } else {
      double s0 = 0., s1 = 0.;
      for (int i = 0; i < m; ++i)
        if (sc->lab[i] == l) {
          if (cnt == 0) { s0 = sc->xs[i]; s1 = sc->ys[i]; }
          else { s0 = __dadd_rn(s0, sc->xs[i]); s1 = __dadd_rn(s1, sc->ys[i]); }
          ++cnt;
        }
      m0 = __ddiv_rn(s0, (double)cnt); m1 = __ddiv_rn(s1, (double)cnt);
    }
    sc->c0[l] = m0; sc->c1[l] = m1; sc->cnt[l] = cnt;
  }
  wave_sync();
  // lanes = members: distance to the own centroid (pairwise_distances' expanded formula)
  if (l < m) {
    const int c = sc->lab[l];
    const double x = sc->xs[l], y = sc->ys[l], m0 = sc->c0[c], m1 = sc->c1[c];
    const double yy = norm2(m0, m1), xxn = norm2(x, y);
    if (pos_f32) {
      double d = __dmul_rn(-2.0, dot2_lo(x, y, m0, m1));
      d = __dadd_rn(d, xxn);
      d = __dadd_rn(d, yy);
      float df = (float)d;
      if (!(df > 0.0f)) df = 0.0f;
      sc->tmpf[l] = sqrtf(df);
    } else {
      double d = __dmul_rn(-2.0, sc->cnt[c] == 1 ? dot2_hi(x, y, m0, m1) : dot2_lo(x, y, m0, m1));
      d = __dadd_rn(d, xxn);
      d = __dadd_rn(d, yy);
      if (!(d > 0.0)) d = 0.0;
      sc->tmp[l] = __dsqrt_rn(d);
    }
  }
  wave_sync();
  // lanes = clusters: the members' distances in member order, their numpy mean
  double* sorted_d = sc->px0;                                       // [NS] doubles or floats
  float* sorted_f = reinterpret_cast<float*>(sc->px0);
  if (l < k) {
    int off = 0;
    for (int c = 0; c < k; ++c) if (c < l) off += sc->cnt[c];
    const int cnt = sc->cnt[l];
    int j = 0;
    for (int i = 0; i < m; ++i)
      if (sc->lab[i] == l) {
        if (pos_f32) sorted_f[off + j] = sc->tmpf[i]; else sorted_d[off + j] = sc->tmp[i];
        ++j;
      }
    double intra;
    if (pos_f32) intra = (double)__fdiv_rn(np_sum_f(sorted_f + off, cnt), (float)cnt);
    else intra = __ddiv_rn(np_sum_d(sorted_d + off, cnt), (double)cnt);
    sc->intra[l] = intra;
  }
  wave_sync();
  if (l < k) sc->tmp[l] = 0.0;                                      // max_b ratio[a][b], filled below (after the fence:
  wave_sync();                                                      // other lanes were still reading tmp[] above)
  const int all_i_zero = __ballot(l < k && !(fabs(sc->intra[l < k ? l : 0]) <= 1e-8)) == 0ull;
  // lanes = b: column b of row a of the ratio matrix; every ratio is a non-negative float64, so the
  // row maximum is the maximum of the bit patterns (LDS 64-bit unsigned max)
  // (lanes = (a, b) pairs, A = 64 / k rows of the matrix per pass: the whole matrix at once for up to 8 clusters)
  int all_d_zero = 1;
  unsigned long long* best_bits = reinterpret_cast<unsigned long long*>(sc->tmp);
  const int rows_per_pass = 64 / k;                                  // k < n <= 64
  const int ar = (int)(((uint32_t)l * (uint32_t)((65536 + k - 1) / k)) >> 16), b = l - ar * k;      // l / k, l % k (exact for l < 64)
  for (int a_base = 0; a_base < k; a_base += rows_per_pass) {
    const int a = a_base + ar;
    bool dnz = false;
    if (ar < rows_per_pass && a < k) {
      const double a0 = sc->c0[a], a1 = sc->c1[a], b0 = sc->c0[b], b1 = sc->c1[b];
      const double na = norm2(a0, a1), nb = norm2(b0, b1);
      double d = __dmul_rn(-2.0, dot2_hi(a0, a1, b0, b1));
      d = __dadd_rn(d, na);
      d = __dadd_rn(d, nb);
      if (!(d > 0.0)) d = 0.0;
      if (a == b) d = 0.0;
      const double D = __dsqrt_rn(d);
      dnz = !(fabs(D) <= 1e-8);
      const double den = (D == 0) ? __longlong_as_double(0x7ff0000000000000ll) : D;
      const double v = __ddiv_rn(__dadd_rn(sc->intra[a], sc->intra[b]), den);
      atomicMax(&best_bits[a], (unsigned long long)__double_as_longlong(v));
    }
    if (__ballot(dnz)) all_d_zero = 0;
  }
  wave_sync();
  if (all_i_zero || all_d_zero) { *score_out = 0.0; return SWB_ENV_ERR_DB_ZERO; }
  const double score = __ddiv_rn(np_sum_d(sc->tmp, k), (double)k);
  *score_out = score;
  wave_sync();
  if (score == 0.0) return SWB_ENV_ERR_DB_ZERO;                      // exactly 0.0 by the regular path: `1. / score` raises too
  return 0;
}

// tasks.py:196-245 Clustering.
template <typename SC>
__device__ __forceinline__ int task_clustering_wave(const swb_task& t, int pos_f32, int n, double px, double py,
                                                    const int8_t* label, SC* sc, double* reward, int* success) {
  double score = 0.0;
  const int err = davies_bouldin_wave(pos_f32, n, px, py, label, sc, &score);
  if (err) { *reward = __longlong_as_double(0x7ff8000000000000ll); *success = 0; return err; }
  const double metric = __ddiv_rn(1.0, score);
  const double dense = __ddiv_rn(__dmul_rn(__dsub_rn(metric, t.termination_threshold), t.reward_range), 2.0);
  const int ok = metric >= t.termination_threshold;
  double r = 0.0;
  if (ok) { r = __dadd_rn(r, t.terminate_bonus); r = __dadd_rn(r, dense); }
  else if (!t.sparse_reward) { r = __dadd_rn(r, dense); }
  *reward = r;
  *success = ok;
  return 0;
}

// task.reward + task.success incl. tasks.py:248-296 MetaAggregated; all lanes, uniform result.
// tv: the task of the episode (task_view_of); sub-task t of it is swb_params::tasks[tv.first() + t], its labels row tv.first() + t.
// n_tasks: tv.n() -- or -1 from a caller that will not use the result (finish_step: no task is evaluated then,
// nothing of the scratch but MetaAggregated's own words is touched, and what comes back is not meaningful).
template <typename TV, typename SC>
__device__ __forceinline__ int eval_task_wave(const swb_params& p, const TV& tv, int n_tasks, int n, double px, double py,
                                              const int8_t* label, SC* sc, double* reward, int* success) {
  const int l = lane_id();
  int err = 0;
  double r0 = 0.0;
  int ok0 = 0;
  for (int t = 0; t < n_tasks; ++t) {
    const swb_task& tk = p.tasks[tv.first() + t];
    const int8_t* lab = label + (tv.first() + t) * p.S;
    double r = 0.0;
    int ok = 0;
    if (tk.kind == SWB_TASK_FIND_GOAL) task_find_goal_wave(tk, n, px, py, lab, sc, &r, &ok);
    else if (tk.kind == SWB_TASK_CLUSTERING) err |= task_clustering_wave(tk, p.pos_is_f32, n, px, py, lab, sc, &r, &ok);
    if (t == 0) { r0 = r; ok0 = ok; }
    if (tv.is_meta() && l == 0) { sc->tr[t] = r; sc->tok[t] = ok; }
  }
  if (!tv.is_meta()) { *reward = r0; *success = ok0; return err; }
  wave_sync();
  const double* r = sc->tr;
  const int* ok = sc->tok;
  int succ = (tv.termination() == SWB_TERM_ALL);
  for (int t = 0; t < n_tasks; ++t) succ = (tv.termination() == SWB_TERM_ALL) ? (succ && ok[t]) : (succ || ok[t]);
  double agg;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (tv.aggregator() == SWB_AGG_SUM || tv.aggregator() == SWB_AGG_MEAN) {
    // np.nansum / np.nanmean over the sub-task rewards (uniform: every lane sums the same values)
    int cnt = 0;
    double v[SWB_MAX_TASKS];
#pragma unroll
    for (int t = 0; t < SWB_MAX_TASKS; ++t) {
      const double x = (t < n_tasks) ? r[t] : 0.0;
      const bool isn = (x != x);
      v[t] = isn ? 0.0 : x;
      cnt += (t < n_tasks) && !isn;
    }
    if (n_tasks < 8) {
      agg = -0.0;
#pragma unroll
      for (int t = 0; t < SWB_MAX_TASKS; ++t) if (t < n_tasks) agg = __dadd_rn(agg, v[t]);
    } else {
      agg = __dadd_rn(__dadd_rn(__dadd_rn(v[0], v[1]), __dadd_rn(v[2], v[3])), __dadd_rn(__dadd_rn(v[4], v[5]), __dadd_rn(v[6], v[7])));
    }
    if (tv.aggregator() == SWB_AGG_MEAN) agg = __ddiv_rn(agg, (double)cnt);
  } else {
    agg = qnan;
    for (int t = 0; t < n_tasks; ++t) {
      if (r[t] != r[t]) continue;
      if (agg != agg) agg = r[t];
      else if (tv.aggregator() == SWB_AGG_MAX ? (r[t] > agg) : (r[t] < agg)) agg = r[t];
    }
  }
  agg = __dadd_rn(agg, __dmul_rn(tv.terminate_bonus(), (double)succ));
  *reward = agg;
  *success = succ;
  wave_sync();
  return err;
}

// --------------------------------------------------------------------------------------------
// The state phase of a step -- everything the reference environment does before a frame is drawn (environment.py step() /
// reset(), action_spaces.py, tasks.py) -- in three pieces: load_env_state, act_and_move, finish_step.  The cover kernel (its P0)
// and the many-sprite state kernel both run these, so there is one copy of the arithmetic.  One wave = one environment.
// --------------------------------------------------------------------------------------------
struct env_state {            // what load_env_state hands on; per lane, lane s < n = sprite s
  bool first, ov;             // (uniform) this step resets the episode; the episode's sprites carry setter overrides
  bool active;                // (uniform) the environment takes part in this step (swb_params::active); else nothing of it changes
  int en, n, sc_old;          // (uniform) pool entry, sprites, steps taken so far
  double px, py;              // position
  double scale_l, ca_l, sa_l, xv_l, yv_l;
  int sh_idx, so_l, nv_l;     // entry of the shape tables; its path's offset and vertex count there (0 for lanes >= n)
  double act;                 // lanes 0..3: the action components
  int acti;                   // lanes 0..1: ... of the embodied action space
};
// what act_and_move hands to finish_step -- and `changed` (wave-uniform): some sprite's position differs BITWISE from the one the
// step began with (false after a missed click, a zero motion, a move clipped back onto the same value, in an environment that
// takes no part in the step -- and on a reset, which moves nothing here: es.first says that)
struct step_cost { double cost; float cost_f32; bool cost_is_f32; int step_count; bool changed; };

// Round 1 of loads (independent of each other): the environment's scalars, its live positions
// and its action.  Round 2 (needs the pool entry): the episode's static sprite columns.
// MASK = false: a caller whose parameter blocks never carry an active mask (the rollout kernels) compiles without the test.
template <bool OV, bool MASK = true, typename SC>
__device__ __forceinline__ env_state load_env_state(const swb_params& p, int env, SC* tscratch) {
  const int l = lane_id();
  const int S = p.S;
  double* gx = p.x + (size_t)env * S;
  double* gy = p.y + (size_t)env * S;
  // (the mask is the caller's input, written by no wave of the launch; one wave-uniform byte, made a scalar before anything
  // branches on it -- gfx950 has no scalar byte load: the compiler loads the one address and takes the first lane)
  bool active = true;
  if constexpr (MASK) { if (p.active != nullptr) active = rfl((int)as_const(p.active)[env]) != 0; }
  // (an environment that takes no part is not reset either: a pending reset stays pending)
  const int rn = (p.render_only || !active) ? 0 : (int)p.reset_next[env];
  const int ep = p.episode[env], pbase = as_const(p.pool_base)[env], plen = as_const(p.pool_len)[env];
  const int en_old = p.entry[env], n_old = p.nspr[env], sc_old = p.step_count[env];
  double px = 0.0, py = 0.0;      // lane s < n holds sprite s's position
  if (l < S) { px = gx[l]; py = gy[l]; }
  // (the small table of shape offsets whole, lane i = entry i: looked up below with cross-lane reads once the shapes are known)
  static_assert(SWB_MAX_SHAPES + 1 <= SWB_WAVE, "one lane per entry of the shape table");
  const int shoff_tab_l = (l <= SWB_MAX_SHAPES) ? p.shape_off[l] : 0;
  double act = 0.0;               // lanes 0..3: the action components
  int acti = 0;
  if (!p.render_only && active) {                       // (the action row of an environment that takes no part is never read)
    if (p.action_space == SWB_ACTION_EMBODIED) { if (l < 2) acti = reinterpret_cast<const int32_t*>(p.actions)[2 * (size_t)env + l]; }
    else if (l < 4) {
      act = p.action_is_f32 ? (double)reinterpret_cast<const float*>(p.actions)[4 * (size_t)env + l]
                            : reinterpret_cast<const double*>(p.actions)[4 * (size_t)env + l];
    }
  }
  const bool first = rn != 0;                           // environment.py:90-91 -> reset() :74-78
  bool ov = false;                                      // this episode's sprites carry setter overrides
  if constexpr (OV) {
    ov = rfl((int)p.ov_flag[env]) != 0;
    if (ov && first) {                                  // a reset draws fresh sprites: the overrides end here
      ov = false;
      if (l == 0) p.ov_flag[env] = 0;
    }
  }
  const int en = rfl(first ? pbase + (ep % plen) : en_old);
  const size_t pe = (size_t)en * S;
  int n = first ? as_const(p.p_n)[en] : n_old;
  int shape_l = 0;
  double scale_l = 1.0, ca_l = 1.0, sa_l = 0.0, xv_l = 0.0, yv_l = 0.0;
  if (l < S) {
    shape_l = p.p_shape[pe + l]; scale_l = p.p_scale[pe + l]; ca_l = p.p_ca[pe + l]; sa_l = p.p_sa[pe + l];
    xv_l = p.p_xv[pe + l]; yv_l = p.p_yv[pe + l];
    if (first) { px = p.p_x[pe + l]; py = p.p_y[pe + l]; gx[l] = px; gy[l] = py; }
    if constexpr (OV) {
      if (ov) { shape_l = p.ov_shape[(size_t)env * S + l]; scale_l = p.ov_scale[(size_t)env * S + l]; }
    }
  }
  if (p.render_only != 1 && active) {                   // (the task's labels: no task is evaluated without a step)
    const int8_t* lab_src = p.p_label + (size_t)en * p.n_tasks * S;
    if constexpr (OV) { if (ov) lab_src = p.ov_label + (size_t)env * p.n_tasks * S; }
    for (int i = l; i < p.n_tasks * S; i += SWB_WAVE) tscratch->labels[i] = lab_src[i];
  }
  n = rfl(n);
  if (first && l == 0) { p.episode[env] = ep + 1; p.entry[env] = en; p.nspr[env] = n; p.step_count[env] = 0; p.reset_next[env] = 0; }
  // lane s: vertex count and offset of sprite s in the shape table
  // (cross-lane reads with every lane active; shape ids are below SWB_MAX_SHAPES: swb_set_pool / the sampler / the setters check)
  const int sh_idx = (int)min((uint32_t)shape_l, (uint32_t)(SWB_MAX_SHAPES - 1));
  const int so_any = __shfl(shoff_tab_l, sh_idx, 64), so_next = __shfl(shoff_tab_l, sh_idx + 1, 64);
  const int so_l = (l < n) ? so_any : 0;
  const int nv_l = (l < n) ? so_next - so_any : 0;
  return env_state{first, ov, active, en, n, sc_old, px, py, scale_l, ca_l, sa_l, xv_l, yv_l, sh_idx, so_l, nv_l, act, acti};
}

// Action decoding, the hit tests (hit(s2, tx, ty): sprite.py:113-115 contains_point of sprite s2 -- wave-uniform -- at the
// offset (tx, ty) from its position), motion, velocities, keep_in_frame: positions move in `es` and in memory.
template <typename HIT>
__device__ __forceinline__ step_cost act_and_move(const swb_params& p, int env, env_state& es, HIT hit) {
  const int l = lane_id(), n = es.n;
  double &px = es.px, &py = es.py;
  double* gx = p.x + (size_t)env * p.S;
  double* gy = p.y + (size_t)env * p.S;
  double cost = 0.0;
  float cost_f32 = 0.0f;
  bool cost_is_f32 = false;
  int step_count = 0;
  bool changed = false;
  if (!p.render_only && !es.first && es.active) {
    const double ox = px, oy = py;
    step_count = es.sc_old + 1;                         // :93
    int moved = -1;
    double m0 = 0.0, m1 = 0.0;
    if (p.action_space == SWB_ACTION_EMBODIED) {        // action_spaces.py:187-214
      const int carry = __builtin_amdgcn_readlane(es.acti, 0), dir = __builtin_amdgcn_readlane(es.acti, 1);
      const double st = p.action_scale;
      if (dir == 0) m1 = st; else if (dir == 1) m0 = -st; else if (dir == 2) m1 = -st; else m0 = st;
      if (n > 0) {
        const int body = n - 1;
        const double bx = readlane_d(px, body), by = readlane_d(py, body);
        if (carry) {                                     // get_carried_sprite :180-185
          for (int s2 = body - 1; s2 >= 0; --s2) {
            const double sx = readlane_d(px, s2), sy = readlane_d(py, s2);
            double tx, ty;
            if (p.pos_is_f32) { tx = (double)__fsub_rn((float)bx, (float)sx); ty = (double)__fsub_rn((float)by, (float)sy); }
            else { tx = __dsub_rn(bx, sx); ty = __dsub_rn(by, sy); }
            if (hit(s2, tx, ty)) {
              moved = s2;
              break;
            }
          }
        }
        if (l == moved || l == body) {
          px = move1(p.pos_is_f32, px, m0, p.keep_in_frame);
          py = move1(p.pos_is_f32, py, m1, p.keep_in_frame);
        }
      }
      cost = __dmul_rn(-p.motion_cost, st);             // :214
    } else {                                             // action_spaces.py:83-104
      const double a0 = readlane_d(es.act, 0), a1 = readlane_d(es.act, 1);
      const double a2 = readlane_d(es.act, 2), a3 = readlane_d(es.act, 3);
      // float32 actions (action_spec() dtype): numpy keeps (a - 0.5) * scale, the motion norm and,
      // against a float32 position, the click offset in float32 (NEP 50); `act` holds them exactly
      const bool af = p.action_is_f32 != 0;
      if (af) {
        const float f0 = (float)a0, f1 = (float)a1, f2 = (float)a2, f3 = (float)a3, sc = (float)p.action_scale;
        float m0f, m1f;
        if (p.action_space == SWB_ACTION_DRAG_AND_DROP) { m0f = __fmul_rn(__fsub_rn(f2, f0), sc); m1f = __fmul_rn(__fsub_rn(f3, f1), sc); }
        else { m0f = __fmul_rn(__fsub_rn(f2, 0.5f), sc); m1f = __fmul_rn(__fsub_rn(f3, 0.5f), sc); }
        m0 = (double)m0f; m1 = (double)m1f;
        cost_f32 = __fmul_rn((float)(-p.motion_cost), sqrtf(__fadd_rn(__fmul_rn(m0f, m0f), __fmul_rn(m1f, m1f))));
        cost = (double)cost_f32;
        cost_is_f32 = true;
      } else if (p.action_space == SWB_ACTION_DRAG_AND_DROP) { // :133-137
        m0 = __dmul_rn(__dsub_rn(a2, a0), p.action_scale); m1 = __dmul_rn(__dsub_rn(a3, a1), p.action_scale);
      } else {                                           // :65-67
        m0 = __dmul_rn(__dsub_rn(a2, 0.5), p.action_scale); m1 = __dmul_rn(__dsub_rn(a3, 0.5), p.action_scale);
      }
      for (int s2 = n - 1; s2 >= 0; --s2) {              // sprites[::-1] :77-81
        const double sx = readlane_d(px, s2), sy = readlane_d(py, s2);
        double tx, ty;
        if (af && p.pos_is_f32) { tx = (double)__fsub_rn((float)a0, (float)sx); ty = (double)__fsub_rn((float)a1, (float)sy); }
        else { tx = __dsub_rn(a0, sx); ty = __dsub_rn(a1, sy); }
        if (hit(s2, tx, ty)) {
          moved = s2;
          break;
        }
      }
      if (l == moved) {
        px = move1(p.pos_is_f32, px, m0, p.keep_in_frame);
        py = move1(p.pos_is_f32, py, m1, p.keep_in_frame);
      }
      if (!af) cost = __dmul_rn(-p.motion_cost, __dsqrt_rn(dot2_hi(m0, m1, m0, m1)));   // :104
    }
    if (l < n) {                                         // update_position :98-99
      px = move1(p.pos_is_f32, px, es.xv_l, p.keep_in_frame);
      py = move1(p.pos_is_f32, py, es.yv_l, p.keep_in_frame);
      gx[l] = px; gy[l] = py;
    }
    changed = __ballot(l < n && (__double_as_longlong(px) != __double_as_longlong(ox) ||
                                 __double_as_longlong(py) != __double_as_longlong(oy))) != 0ull;
  }
  return step_cost{cost, cost_f32, cost_is_f32, step_count, changed};
}

// The environment's task record (swb_params::task_cache) joins the state phase's first round of loads -- its address depends on
// `env` alone -- and waits in the scratch's `pres` words, idle until a clustering is evaluated, not in registers across the hit
// tests.  A plain load: this wave may write the record again in finish_step.  Two halves around load_env_state: the load is issued
// before the state's own, the word goes to LDS behind them -- written where it is loaded, the LDS store waits for the load with
// nothing else in flight, one more memory round trip at the head of every wave (measured: +1.1 us on a single-round launch).
__device__ __forceinline__ uint32_t load_task_record(const swb_params& p, int env) {
  const int l = lane_id();
  uint32_t w = 0u;                                      // lane l < 4: word l of the record
  if (p.task_cache != nullptr && l < 4) w = reinterpret_cast<const uint32_t*>(p.task_cache)[4 * (size_t)env + l];
  return w;
}
template <typename SC>
__device__ __forceinline__ void park_task_record(const swb_params& p, uint32_t w, SC* tscratch) {
  static_assert(sizeof(SC::pres) == sizeof(swb_task_record), "the record waits in task_scratch::pres");
  if (p.task_cache != nullptr && lane_id() < 4) tscratch->pres[lane_id()] = w;
}

// The task of the episode in pool entry `en` (wave-uniform).  Only the SETS builds (swb_cover_sets_kernel, swb_ms_state_sets_kernel) look a task set up (behind swb_params::ov_flag): the
// others are the kernels of handles without task sets, and take the config block as constants of the launch.
template <bool SETS>
__device__ __forceinline__ task_view<SETS> task_view_of(const swb_params& p, int en) {
  if constexpr (SETS) {
    task_view<true> v{0, p.n_tasks, p.is_meta, p.meta_aggregator, p.meta_termination, p.max_episode_length, p.meta_terminate_bonus};
    // (pointer, byte and record are the host's, written by no wave -- the pointer's line holds no flag --: uniform loads through
    // the constant address space, the byte made a scalar as the mask's is)
    const uint8_t* const p_set = *as_const(reinterpret_cast<const uint8_t* const*>(p.ov_flag + SWB_OV_SLOT(p.N)));
    if (p_set != nullptr) {
      const int g = min(rfl((int)as_const(p_set)[SWB_SET_TABLE_BYTES + (size_t)en]), SWB_MAX_TASK_SETS - 1);
      static_assert(sizeof(swb_task_set) == 32 && offsetof(swb_task_set, meta_terminate_bonus) == 24, "six ints and a double");
      const auto w = as_const(reinterpret_cast<const int32_t*>(p_set)) + 8 * g;
      const double bonus = as_const(reinterpret_cast<const double*>(p_set))[4 * g + 3];
      v = task_view<true>{w[0], w[1], w[2], w[3], w[4], w[5], bonus};
    }
    return v;
  } else {
    return task_view<false>{p};
  }
}

// Task reward / success (spread over the lanes), out-of-frame, termination; the outputs of the step.  Returns the error
// bits of the environment (lane 0; the caller stores them).
// CACHE (swb_params::task_cache; the caller has run stage_task_record): a step that is no reset and moved no sprite takes the
// task's reward, success and error bits from the environment's record when it carries the launch's epoch -- the error bits as
// a fresh evaluation would return them (p.error is sticky and the caller may have cleared it); every other step evaluates and
// leaves the record.  CACHE = false: a caller on forked parameter blocks (the rollout kernels) compiles all of it out.
template <bool OV, bool CACHE = true, bool SETS = false, typename SC>
__device__ __forceinline__ uint32_t finish_step(const swb_params& p, int env, const env_state& es, const step_cost& c, SC* tscratch) {
  const int l = lane_id(), S = p.S, n = es.n;
  const double px = es.px, py = es.py;
  const task_view<SETS> tv = task_view_of<SETS>(p, es.en);
  wave_sync();
  // tasks.py:134-137, 196-205: `contains(sprite.factors)` is evaluated at every step and x / y are factors -- a task whose
  // filter keys on position takes every sprite's label from the cell of the task's grid the sprite stands in NOW (lanes =
  // sprites; swb_task::xcuts / ycuts: the comparisons are numpy's, the bounds already rounded to the position dtype)
  if (p.p_cell_label != nullptr) {                     // (wave-uniform; no shipped configuration)
    const int8_t* cells = p.p_cell_label + (size_t)es.en * p.n_tasks * S * SWB_MAX_CELLS;
    if constexpr (OV) { if (es.ov && p.ov_cell_label) cells = p.ov_cell_label + (size_t)env * p.n_tasks * S * SWB_MAX_CELLS; }
    for (int t = tv.first(); t < tv.first() + tv.n(); ++t) {
      const swb_task& tk = p.tasks[t];
      if (tk.n_xcuts + tk.n_ycuts == 0) continue;
      if (l < n) {
        int cx = 0, cy = 0;
        for (int k = 0; k < tk.n_xcuts; ++k) cx += (px >= tk.xcuts[k]) ? 1 : 0;
        for (int k = 0; k < tk.n_ycuts; ++k) cy += (py >= tk.ycuts[k]) ? 1 : 0;
        tscratch->labels[t * S + l] = cells[((size_t)t * S + l) * SWB_MAX_CELLS + cy * (tk.n_xcuts + 1) + cx];
      }
    }
    wave_sync();
  }
  const bool oof_l = (l < n) && !(px >= 0. && py >= 0. && px <= 1. && py <= 1.);   // sprite.py:135-138
  const int oof = __ballot(oof_l) != 0ull;
  double tr = 0.0; int ok = 0;
  // (A wave that reuses its record runs the evaluation over a task count of -1 instead of branching around it: the task loop
  // has a run-time trip count already, so the kernel's control flow -- and with it the register allocation of the cover builds,
  // which a branch around the whole evaluation cost two spilled VGPRs each -- stays what it was.  No fence is needed between
  // the stamp's read and an evaluation's writes to `pres`: the loop is entered on a count that depends on the value read.)
  int n_tasks = tv.n();                                 // (wave-uniform; -1: the record is reused)
  if constexpr (CACHE) {
    if (p.task_cache != nullptr) {
      // (every lane reads the same word and decides the same; the decision goes through a ballot so that the compiler KNOWS the
      // count is uniform -- `changed` and `first` are set under branches it takes for divergent -- and the task loop stays scalar)
      const uint32_t stamp = tscratch->pres[3];
      if (__ballot(stamp != p.task_epoch || c.changed || es.first) == 0ull) n_tasks = -1;
    }
  }
  int terr = eval_task_wave(p, tv, n_tasks, n, px, py, tscratch->labels, tscratch, &tr, &ok);
  const bool reuse = CACHE && n_tasks < 0;
  if constexpr (CACHE) {
    if (reuse) {                                        // (no task ran: `pres` still holds the record)
      const uint32_t w0 = tscratch->pres[0], w1 = tscratch->pres[1], w2 = tscratch->pres[2];
      tr = __longlong_as_double((long long)(((unsigned long long)w1 << 32) | w0));
      ok = (int)(w2 & 0xffu);
      terr = (int)((w2 >> 8) & 0xffu);
    }
  }
  if (l == 0) {
    if constexpr (CACHE) {
      if (p.task_cache != nullptr && !reuse) {          // (one 16-byte vector store; only where the task was in fact evaluated)
        const unsigned long long trb = (unsigned long long)__double_as_longlong(tr);
        uint4 rec;
        rec.x = (uint32_t)trb; rec.y = (uint32_t)(trb >> 32);
        rec.z = (uint32_t)(ok & 0xff) | ((uint32_t)(terr & 0xff) << 8);
        rec.w = p.task_epoch;
        *reinterpret_cast<uint4*>(&p.task_cache[env]) = rec;
      }
      if (p.task_stats != nullptr) atomicAdd(&p.task_stats[reuse ? 0 : 1], 1ull);
    }
    if (p.success) p.success[env] = (uint8_t)ok;
    if (p.render_only) {
      // (swb_evaluate: environment.py:80-81 success() of the current sprites, no time step)
    } else if (es.first) {
      if (p.reward) p.reward[env] = __longlong_as_double(0x7ff8000000000000ll);
      if (p.discount) p.discount[env] = __int_as_float(0x7fc00000);
      if (p.step_type) p.step_type[env] = SWB_STEP_FIRST;
    } else {
      // :101 reward += task.reward.  A float32 cost plus a Python-float task reward (NoReward,
      // Clustering) stays float32 under NEP 50; np.float64 rewards promote to float64.
      const bool task_is_pyfloat = !tv.is_meta() && p.tasks[tv.first()].kind != SWB_TASK_FIND_GOAL;
      const double rew = (c.cost_is_f32 && task_is_pyfloat) ? (double)__fadd_rn(c.cost_f32, (float)tr) : __dadd_rn(c.cost, tr);
      if (p.reward) p.reward[env] = rew;
      // (:84.  Two copies of one expression ON PURPOSE: behind the accessor the compiler hoists the plain builds' load of
      // max_episode_length out of the short-circuit below, and they would no longer be, instruction for instruction, the kernels
      // they were before task sets -- which is checked by diffing their assembly, profiles/r25_task_sets.md.  Do not fold.)
      int timeout;
      if constexpr (SETS) timeout = c.step_count >= tv.max_episode_length();
      else timeout = c.step_count >= p.max_episode_length;
      const int last = ok || oof || timeout;                             // :104-106
      p.step_count[env] = c.step_count;
      if (last) p.reset_next[env] = 1;
      if (p.step_type) p.step_type[env] = last ? SWB_STEP_LAST : SWB_STEP_MID;
      if (p.discount) p.discount[env] = last ? 0.0f : 1.0f;
    }
  }
  return l == 0 ? (uint32_t)terr : 0u;
}

// --------------------------------------------------------------------------------------------
// LDS layout (per wave)
// --------------------------------------------------------------------------------------------
struct edge_rec {        // 16 bytes; canvas coordinates must fit int16 (else SWB_ENV_ERR_SPAN_OVERFLOW)
  int16_t x0, y0, y1;
  int16_t xtop;          // replacement crossing at the top end ("discontiguous corners"), an integer
  float dx;              // slope; for a horizontal edge (y0 == y1) the bits hold x1 instead
  int16_t xbot;          // ... at the bottom end on the polygon's last row; SWB_NO_REPL = none
  int16_t pad;
};
#define SWB_NO_REPL (-32768)

__device__ __forceinline__ float repl_to_float(int v) { return v == SWB_NO_REPL ? __int_as_float(0x7fc00000) : (float)v; }
__device__ __forceinline__ int repl_to_int(float v) { return (v == v) ? (int)v : SWB_NO_REPL; }

struct sprite_rec {      // per sprite, wave-uniform
  int32_t edge_off, n_edges;
  int32_t ymin, ymax;    // clamped scan range [max(min,0), min(max,Hc)]
  uint32_t rgb;
  int32_t w0, w1;        // 32-pixel words of the canvas row the sprite can touch
  int32_t max_edge_rows; // longest edge, in canvas rows (chooses the lane mapping of P2)
};

// The row masks cover a window of NWA 32-pixel words (160 px on canvases up to 320 px, else 192 px);
// a sprite wider than that is scan-converted in several x-chunks.
#define SWB_NWA(NW) ((NW) <= 5 ? (NW) : ((NW) <= 10 ? 5 : 6))
template <int NW>
struct wave_lds {
  // masks[w][lane]: parity toggles T and crossing pixels Px for the current (batch, sprite, chunk)
  uint32_t T[SWB_NWA(NW)][SWB_WAVE];
  uint32_t Px[SWB_NWA(NW)][SWB_WAVE];
  sprite_rec spr[SWB_TUNED_SPRITES];
  int32_t ovf_slot;                         // this wave's HBM overflow slot: -1 none yet, -2 none free
  int32_t pad_[3];
  uint32_t outrow[];                        // [outrow_bytes / 4] packed-byte staging of one output row; P1b scratch (132 ints)
  // dynamic tail: edge_rec edges[max_edges]; uint32_t spans[M][64] (spans[m][row] = start |
  // end<<10 | sprite<<20), whose storage doubles as the task_scratch of P0
};

// --------------------------------------------------------------------------------------------
// P1b: canvas edges of all sprites at once, pil_renderer.py:80-83 + Pillow ImagingDrawPolygon: lanes =
// polygon vertices / edges of the whole scene, 64 per pass (one sprite per pass, as in round 1, leaves
// most lanes idle for squares and triangles and pays its fixed cost once per sprite):
//   sweep 1  vertices -> canvas ints (stored in the x0/y0 fields of the edge records, with the
//            owning sprite and the local vertex index in `pad`)
//   sweep 2  edges: end point, float32 slope, per-sprite extents through LDS atomics
//   sweep 3  the "connect discontiguous corners" rule for both ends of every edge: closed-form
//            partner when the sprite provably has no two vertices on one integer point, else the
//            scan over all earlier edges of the sprite.
// "Provably": two vertices whose canvas distance is >= 2*sqrt(2) differ by >= 2 in x or in y and
// cannot truncate to the same integer; the smallest vertex distance of each shape at unit scale
// is a host-computed table (shape_dmin).  The test is conservative: it may send a sprite without
// duplicates to the general scan, which gives the same result.
// Edge k of sprite s lives in slot voff_s + k (its first vertex's slot).
// --------------------------------------------------------------------------------------------
struct corner_end {          // one end of an edge in the corner rule
  int row, adj;
  float xc, repl;
  bool live;
};
__device__ __forceinline__ void corner_try(corner_end& c, int cx0, int cy0, float cdx, int ox0, int oy0, int oy1, float odx,
                                           bool want) {
  if (want) {
    const int oymin = min(oy0, oy1), oymax = max(oy0, oy1);
    const float xo = pil_cross(c.row, oy0, odx, ox0);
    if (roundf(c.xc) == roundf(xo) && c.adj >= oymin && c.adj <= oymax) {
      const float a = pil_cross(c.adj, cy0, cdx, cx0);
      const float b = pil_cross(c.adj, oy0, odx, ox0);
      if (c.xc > __fadd_rn(a, 1.0f) && c.xc > __fadd_rn(b, 1.0f)) c.repl = __fadd_rn(roundf(fmaxf(a, b)), 1.0f);
      else if (c.xc < __fsub_rn(a, 1.0f) && c.xc < __fsub_rn(b, 1.0f)) c.repl = __fsub_rn(roundf(fminf(a, b)), 1.0f);
      c.live = false;                                    // first matching earlier edge wins
    }
  }
}

// rowtab: SWB_ROWTAB_DWORDS dwords of scratch (the span lists, idle until P2) -- for the general scan, per sprite and per
// canvas row modulo 8 the edges that have an end on such a row.
#define SWB_ROWTAB_SLOTS 8
#define SWB_ROWTAB_DWORDS (SWB_TUNED_SPRITES * SWB_ROWTAB_SLOTS * 2)
static_assert(SWB_ROWTAB_DWORDS * 4 <= SWB_MIN_SPANS * 256, "the row table borrows the span lists");
template <int NW>
__device__ __forceinline__ void build_all_edges(const swb_params& p, wave_lds<NW>* L, edge_rec* edges, const double2* cpath,
                                                uint32_t* rowtab, int nspr, int vtotal, int voff_l, int nv_l, double px, double py,
                                                double dmin_l, double scale_l, uint32_t rgb_reg, uint32_t& err) {
  const int l = lane_id();
  double* posx = reinterpret_cast<double*>(L->outrow);                 // [16] sprite positions
  double* posy = posx + SWB_TUNED_SPRITES;                              // [16]
  int* nvs = reinterpret_cast<int*>(posy + SWB_TUNED_SPRITES);          // [16] vertex counts
  int* flags = nvs + SWB_TUNED_SPRITES;                                 // [16] 1: general corner scan
  int* misc = flags + SWB_TUNED_SPRITES;                                // (4 dwords of padding)
  uint32_t* umask = reinterpret_cast<uint32_t*>(misc + 4);              // [16][2] bit i: edge i of the sprite can be a partner
  if (l < nspr) {
    posx[l] = px; posy[l] = py; nvs[l] = nv_l;
    sprite_rec r;
    r.edge_off = voff_l; r.n_edges = 0; r.ymin = 0x7fffffff; r.ymax = -0x7fffffff; r.rgb = rgb_reg;
    r.w0 = 0x7fffffff; r.w1 = -0x7fffffff; r.max_edge_rows = 0;        // w0/w1 hold min/max x until finalised
    L->spr[l] = r;
  }
  if (l < 2 * SWB_TUNED_SPRITES) umask[l] = 0u;
  // corner-rule mode of every sprite (see the header): can two of its vertices share a pixel?
  const bool nodup_l = __dmul_rn(__dmul_rn(dmin_l, scale_l), (double)min(p.Wc, p.Hc)) >= 2.9;
  if (l < nspr) flags[l] = nodup_l ? 0 : 1;
  const bool any_general = __ballot(l < nspr && !nodup_l) != 0ull;
  if (any_general) {
    static_assert(SWB_ROWTAB_DWORDS == 4 * SWB_WAVE, "four dwords per lane");
#pragma unroll
    for (int k = 0; k < 4; ++k) rowtab[k * SWB_WAVE + l] = 0u;
  }
  wave_sync();
  // ---- sweep 1: vertices -> canvas ints (C truncation)
  for (int base = 0; base < vtotal; base += 64) {
    const int k = base + l;
    int sid = 0, vb = 0;
    for (int s2 = 1; s2 < nspr; ++s2) {
      const int v = __builtin_amdgcn_readlane(voff_l, s2);
      if (k >= v) { sid = s2; vb = v; }
    }
    if (k < vtotal) {
      const double cx = cpath[k].x, cy = cpath[k].y;
      const double sx = posx[sid], sy = posy[sid];
      // sprite.py:131-133 translate: (1*x + 0*y) + px
      const double vx = __dadd_rn(__dadd_rn(__dmul_rn(1.0, cx), __dmul_rn(0.0, cy)), sx);
      const double vy = __dadd_rn(__dadd_rn(__dmul_rn(0.0, cx), __dmul_rn(1.0, cy)), sy);
      // The range is decided on the doubles: converting one that is NaN or outside int is undefined (x86 gives INT_MIN, gfx950
      // saturates and turns NaN into 0), and |trunc(v)| <= 32000 is |v| < 32001.  NaN fails the comparison; a vertex that
      // fails is flagged and stored as 0, so that every later phase sees coordinates that fit the records.
      const double fx = __dmul_rn((double)p.Wc, vx), fy = __dmul_rn((double)p.Hc, vy);
      const bool fits = fabs(fx) < SWB_TUNED_COORD_LIMIT + 1.0 && fabs(fy) < SWB_TUNED_COORD_LIMIT + 1.0;
      if (!fits) err |= SWB_ENV_ERR_SPAN_OVERFLOW;
      const int X = fits ? (int)fx : 0, Y = fits ? (int)fy : 0;
      edge_rec e;
      e.x0 = (int16_t)X; e.y0 = (int16_t)Y; e.y1 = 0; e.xtop = SWB_NO_REPL; e.dx = 0.0f; e.xbot = SWB_NO_REPL;
      e.pad = (int16_t)(sid | ((k - vb) << 8));
      edges[k] = e;
    }
  }
  wave_sync();
  // closing edge n-1 -> 0 only if the end points differ
  if (l < nspr) {
    const edge_rec f = edges[voff_l], g = edges[voff_l + nv_l - 1];
    L->spr[l].n_edges = (g.x0 != f.x0 || g.y0 != f.y0) ? nv_l : nv_l - 1;
  }
  wave_sync();
  // ---- sweep 2: edges
  for (int base = 0; base < vtotal; base += 64) {
    const int k = base + l;
    if (k < vtotal) {
      const edge_rec e = edges[k];
      const int sid = e.pad & 255, i = e.pad >> 8;
      const int n = nvs[sid], ne = L->spr[sid].n_edges, vb = L->spr[sid].edge_off;
      if (i < ne) {
        const edge_rec e1 = edges[(i + 1 == n) ? vb : k + 1];
        const int x0 = e.x0, y0 = e.y0, x1 = e1.x0, y1 = e1.y0;
        float dx = 0.0f;
        if (y0 != y1) dx = __fdiv_rn((float)(x1 - x0), (float)(y1 - y0));
        const int eymin = min(y0, y1), eymax = max(y0, y1);
        atomicMin(&L->spr[sid].ymin, eymin); atomicMax(&L->spr[sid].ymax, eymax);
        atomicMin(&L->spr[sid].w0, min(x0, x1)); atomicMax(&L->spr[sid].w1, max(x0, x1));
        atomicMax(&L->spr[sid].max_edge_rows, eymax - eymin + 1);
        edges[k].y1 = (int16_t)y1;
        edges[k].dx = (y0 == y1) ? __int_as_float(x1) : dx;
        // (corner rule: only non-horizontal, non-vertical edges are in Pillow's table of partners)
        if (y0 != y1 && dx != 0.0f && i < 64) {
          atomicOr(&umask[2 * sid + (i >> 5)], 1u << (i & 31));
          if (flags[sid]) {                      // general scan: a partner must have an end on the row of the end it serves
            atomicOr(&rowtab[(sid * SWB_ROWTAB_SLOTS + (y0 & (SWB_ROWTAB_SLOTS - 1))) * 2 + (i >> 5)], 1u << (i & 31));
            atomicOr(&rowtab[(sid * SWB_ROWTAB_SLOTS + (y1 & (SWB_ROWTAB_SLOTS - 1))) * 2 + (i >> 5)], 1u << (i & 31));
          }
        }
      }
    }
  }
  wave_sync();
  // per sprite: scan range (Draw.c: ymin starts at ysize-1, ymax at 0), word extent, corner-rule mode
  if (l < nspr) {
    sprite_rec r = L->spr[l];
    int ymin = min(r.ymin, p.Hc - 1), ymax = max(r.ymax, 0);
    if (ymin < 0) ymin = 0;
    if (ymax > p.Hc) ymax = p.Hc;
    // horizontal extent: every crossing, rounded, lies within [min x - 1, max x + 1]; the parity
    // toggle sits one pixel further right and a corner replacement at most one further out.
    const int sxmin = r.w0, sxmax = r.w1;
    r.ymin = ymin; r.ymax = ymax;
    r.w0 = min(max((sxmin - 3) >> 5, 0), NW - 1);
    r.w1 = min(max((sxmax + 4) >> 5, 0), NW - 1);
    L->spr[l] = r;
  }
  wave_sync();
  // ---- sweep 3: "connect discontiguous corners" for the top end (row edge.ymin) and the bottom
  // end (row edge.ymax, only when it is the polygon's last row) of every edge
  for (int base = 0; base < vtotal; base += 64) {
    const int k = base + l;
    const bool valid = k < vtotal;
    edge_rec e;
    e.x0 = e.y0 = e.y1 = 0; e.dx = 0.f; e.xtop = e.xbot = SWB_NO_REPL; e.pad = 0;
    if (valid) e = edges[k];
    const int sid = e.pad & 255, i = e.pad >> 8;
    const int n = nvs[sid], ne = L->spr[sid].n_edges, vb = L->spr[sid].edge_off, symax = L->spr[sid].ymax;
    const bool general = flags[sid] != 0;
    const bool have = valid && i < ne;
    const int cx0 = e.x0, cy0 = e.y0, cy1 = e.y1;
    const float cdx = e.dx;
    const int cymin = min(cy0, cy1), cymax = max(cy0, cy1);
    const bool base_live = have && (cy0 != cy1) && (cdx != 0.0f);
    corner_end top, bot;
    top.row = cymin; top.adj = cymin + 1; top.live = base_live;
    bot.row = cymax; bot.adj = cymax - 1; bot.live = base_live && (cymax == symax);
    top.xc = pil_cross(top.row, cy0, cdx, cx0); bot.xc = pil_cross(bot.row, cy0, cdx, cx0);
    top.repl = bot.repl = __int_as_float(0x7fc00000);
    // Partner search.  The rule needs an EARLIER, non-vertical edge j < i that also ends on `row` and
    // whose crossing there rounds to the same pixel, i.e. an edge incident to the same integer end
    // point.  Without duplicate vertices the only edges incident to a vertex are its two polygon
    // edges: at most one candidate, known in closed form.
    if (__ballot(!general && (top.live || bot.live))) {
#pragma unroll
      for (int end = 0; end < 2; ++end) {
        corner_end& c = end ? bot : top;
        const bool at_start = (c.row == cy0);
        int kl = at_start ? i - 1 : ((i + 1 == n) ? 0 : i + 1);
        const bool earlier = (kl >= 0) && (kl < i) && (kl < ne);
        kl = max(kl, 0);
        const bool want0 = !general && c.live && earlier;
        edge_rec o;
        o.x0 = o.y0 = o.y1 = 0; o.dx = 0.f; o.xtop = o.xbot = SWB_NO_REPL; o.pad = 0;
        if (want0) o = edges[vb + kl];
        const int oy0 = o.y0, oy1 = o.y1;
        corner_try(c, cx0, cy0, cdx, o.x0, oy0, oy1, o.dx,
                   want0 && oy0 != oy1 && o.dx != 0.0f && (c.row == oy0 || c.row == oy1));
      }
    }
    // General scan (sprites whose vertices may share pixels): the earlier edges j < i of the sprite in ascending order, first
    // match wins.  Only edges that can be partners at all (umask: a third of a tiny 30-gon's) AND have an end on the row of
    // one of this edge's live ends (rowtab, rows modulo 8: a quarter of those again) are visited, each lane walking its own
    // candidate bits; a lane is done when both ends are settled.
    if (any_general) {
      unsigned long long cand = 0ull;
      if (general && (top.live || bot.live)) {
        const int upto = min(i, ne - 1);                             // j < i and j < ne - 1
        const unsigned long long um = (unsigned long long)umask[2 * sid] | ((unsigned long long)umask[2 * sid + 1] << 32);
        const uint32_t* rt = rowtab + (sid * SWB_ROWTAB_SLOTS + (top.row & (SWB_ROWTAB_SLOTS - 1))) * 2;
        const uint32_t* rb = rowtab + (sid * SWB_ROWTAB_SLOTS + (bot.row & (SWB_ROWTAB_SLOTS - 1))) * 2;
        const unsigned long long on_rows = (top.live ? ((unsigned long long)rt[0] | ((unsigned long long)rt[1] << 32)) : 0ull) |
                                           (bot.live ? ((unsigned long long)rb[0] | ((unsigned long long)rb[1] << 32)) : 0ull);
        cand = (upto >= 64 ? um : (um & ((1ull << max(upto, 0)) - 1ull))) & on_rows;
      }
      while (__ballot(cand != 0ull)) {
        const bool mine = cand != 0ull;
        const int j = mine ? __builtin_ctzll(cand) : 0;
        cand &= cand - 1ull;                                          // (0 stays 0)
        edge_rec o;
        o.x0 = o.y0 = o.y1 = 0; o.dx = 0.f; o.xtop = o.xbot = SWB_NO_REPL; o.pad = 0;
        if (mine) o = edges[vb + j];
        const int oy0 = o.y0, oy1 = o.y1;
        const bool wt = mine && top.live && (top.row == oy0 || top.row == oy1);
        const bool wb = mine && bot.live && (bot.row == oy0 || bot.row == oy1);
        if (__ballot(wt || wb)) {                                     // (else: no lane's end row is an end row of its edge j)
          corner_try(top, cx0, cy0, cdx, o.x0, oy0, oy1, o.dx, wt);
          corner_try(bot, cx0, cy0, cdx, o.x0, oy0, oy1, o.dx, wb);
        }
        if (!(top.live || bot.live)) cand = 0ull;
      }
    }
    if (have) {
      edges[k].xtop = (int16_t)repl_to_int(top.repl);
      edges[k].xbot = (int16_t)repl_to_int(bot.repl);
    }
  }
  wave_sync();
}

// --------------------------------------------------------------------------------------------
// Span lists of the canvas rows of a batch (filled by P2, read by P3).
// --------------------------------------------------------------------------------------------
// Visible spans of a canvas row: the SWB_REG_SPANS most recent stay in the registers of the lane that
// owns the row (fetched later with v_readlane, no LDS round trip), older ones in LDS (M per row), the
// rest (virtually never) in an HBM overflow slot.
#define SWB_REG_SPANS 3
struct row_spans {
  uint32_t cnt, s0, s1, s2;
};
// HBM overflow of the span lists.  A wave that needs it takes a slot from the bitmap (lane 0, at a
// convergent point of the kernel: see coverage_with_overflow) and gives it back at kernel end; the slot
// index lives in LDS.  put_span itself never allocates: without a slot it drops the span and raises
// SWB_INT_NEED_SLOT, and the batch is scanned again once the slot is there.
#define SWB_INT_NEED_SLOT 0x80u          // internal bit of `err`, never stored
#define SWB_EAGER_OVF_SPRITES 8
__device__ __forceinline__ int ovf_slot_alloc(const swb_params& p) {
  // Waves resident at the same time have (mostly) consecutive block indices: spreading them over the words
  // by index, and over the bits of a word by the next index digits, keeps the retries near zero while the
  // bitmap is at most half full (swb.hip sizes it at twice the resident waves).
  const int nw = p.ovf_slots >> 5;
  int w = (int)(blockIdx.x % (uint32_t)nw);
  const int rot = (int)((blockIdx.x / (uint32_t)nw) & 31u);
  for (int tries = 0; tries < 2 * nw; ++tries) {
    uint32_t cur = __hip_atomic_load(&p.ovf_bitmap[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (~cur) {
      const uint32_t freeb = ~cur;
      const uint32_t at_or_after = freeb & (0xffffffffu << rot);          // first free bit at or after `rot`, else any
      const uint32_t bit = 1u << (__ffs((int)(at_or_after ? at_or_after : freeb)) - 1);
      const uint32_t old = atomicOr(&p.ovf_bitmap[w], bit);
      if (!(old & bit)) return 32 * w + (__ffs((int)bit) - 1);
      cur = old | bit;
    }
    w = (w + 1 == nw) ? 0 : w + 1;
  }
  return -2;
}
__device__ __forceinline__ void ovf_slot_release(const swb_params& p, int32_t* slot_lds) {   // lane 0, end of kernel
  const int s = *slot_lds;
  if (s >= 0) atomicAnd(&p.ovf_bitmap[s >> 5], ~(1u << (s & 31)));
}

// The registers hold the row's three most recent spans (a new one shifts in, no index compares); the
// span that falls out goes to the LDS list, then to the HBM slot.  The order of a row's spans is
// irrelevant to its consumers (the horizontal pass sums over them, they are disjoint).
__device__ __forceinline__ void put_span(const swb_params& p, uint32_t* spans, int32_t* ovf, row_spans& rs, int row,
                                         uint32_t v, uint32_t& err) {
  const uint32_t m = rs.cnt;
  if (m >= SWB_REG_SPANS) {
    const uint32_t k = m - SWB_REG_SPANS;
    if (k < (uint32_t)p.span_cap) spans[k * SWB_WAVE + row] = rs.s2;
    else if (k - p.span_cap < (uint32_t)p.ovf_cap) {
      const int s = *(volatile int32_t*)ovf;
      if (s >= 0) p.ovf[((size_t)s * 64 + row) * p.ovf_cap + (k - p.span_cap)] = rs.s2;
      else err |= SWB_INT_NEED_SLOT;
    } else err |= SWB_ENV_ERR_SPAN_OVERFLOW;
  }
  rs.s2 = rs.s1; rs.s1 = rs.s0; rs.s0 = v;
  rs.cnt = m + 1;
}
__device__ __forceinline__ uint32_t get_span(const swb_params& p, const uint32_t* spans, const int32_t* ovf,
                                             const row_spans& rs, int m, int row) {
  if (m == 0) return (uint32_t)__builtin_amdgcn_readlane((int)rs.s0, row);
  if (m == 1) return (uint32_t)__builtin_amdgcn_readlane((int)rs.s1, row);
  if (m == 2) return (uint32_t)__builtin_amdgcn_readlane((int)rs.s2, row);
  uint32_t v = 0u;                                  // (an empty span when no overflow slot could be had)
  if (m - SWB_REG_SPANS < p.span_cap) v = spans[(m - SWB_REG_SPANS) * SWB_WAVE + row];
  else {
    const int s = rfl(*ovf);
    if (s >= 0) v = p.ovf[((size_t)s * 64 + row) * p.ovf_cap + (m - SWB_REG_SPANS - p.span_cap)];
  }
  return (uint32_t)rfl((int)v);
}

// Horizontal edge (Draw.c: hline(xmin, y0, xmax) drawn up front): pixels [a, b] of row column rl.
template <int NW>
__device__ __forceinline__ void scatter_hline(wave_lds<NW>* L, int xb, int npx, int rl, int a, int b) {
  a -= xb; b -= xb;
  if (a < npx && b >= 0) {
    a = max(a, 0); b = min(b, npx - 1);
    for (int w = a >> 5; w <= (b >> 5); ++w) {
      const int lo = max(a - 32 * w, 0), hi = min(b - 32 * w, 31);
      atomicOr(&L->Px[w][rl], (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo));
    }
  }
}

// --------------------------------------------------------------------------------------------
// P2: coverage of one batch of 64 canvas rows.  Pillow polygon_generic (Draw.c), see oracle/sw_oracle.c
// polygon_generic for the rule; here the sorted even-odd pairing is expressed without sorting:
//   painted(x) = parity(#{crossings with ROUND_DOWN < x}) | (x in [ROUND_UP, ROUND_DOWN] of some
//   crossing) | (x on a horizontal edge of this row).
// The code is written for the instruction budget (the kernel is bound by vector AND scalar issue):
//   * the sprites that intersect the batch come from a ballot over per-sprite lane registers
//     (front to back = highest set bit first) instead of seven LDS reads per sprite and batch;
//   * one (edge, row) crossing is straight-line code: lanes without a toggle / crossing pixel
//     issue the LDS xor / or with a zero mask instead of branching around it (the round-1 version
//     spent as many scalar instructions on exec-mask bookkeeping as vector instructions on
//     arithmetic), the float64 rounding of negative crossings is entered only when some lane has one;
//   * shapes with many short edges (the 30-gon) give every edge G = 2^k <= 64 / n_edges lanes that
//     walk its rows with stride G, instead of one lane per edge;
//   * the word loop tests one precomputed bit per canvas word.
// --------------------------------------------------------------------------------------------
template <int NW>
__device__ __forceinline__ void scatter_crossing2(wave_lds<NW>* L, int xb, int npx, int rl, bool act, int y, float x0f, int y0,
                                                  float dx, float xtop, float xbot, bool any_repl, bool maybe_neg, int eymin,
                                                  int eymax, int symax, bool left_acts = true) {
  float xx = __fadd_rn(__fmul_rn((float)(y - y0), dx), x0f);           // Draw.c: (y - y0) * dx + x0, float32, no FMA
  const bool dup = (y == eymax) && (y < symax);
  if (any_repl) {                                                      // wave-uniform: some lane's edge has a corner replacement
    const bool rep = !dup && dx != 0.0f;
    if (rep && y == eymin) { if (xtop == xtop) xx = xtop; }
    else if (rep && y == eymax) { if (xbot == xbot) xx = xbot; }
  }
  int ru, rd;
  // (a crossing can only be negative for a sprite that reaches the first canvas word: `maybe_neg`, wave-uniform)
  // Draw.c rounds negative values away from zero, so a negative half has ROUND_UP = ROUND_DOWN - 1: of those two
  // pixels only ROUND_DOWN can be on the canvas (pixel 0, for x = -0.5)
  if (maybe_neg && __ballot(act && xx < 0.0f)) { rd = pil_round_down(xx); ru = max(pil_round_up(xx), rd); }
  else { ru = (int)floorf(__fadd_rn(xx, 0.5f)); rd = (int)ceilf(__fsub_rn(xx, 0.5f)); }
  uint32_t* Tcol = &L->T[0][0] + rl;
  uint32_t* Pcol = &L->Px[0][0] + rl;
  // parity toggle at ROUND_DOWN + 1 (a duplicated crossing toggles twice: none); one left of the
  // window acts at its first pixel, one right of it not at all.  (left_acts = false, wave-uniform: this is a later x-chunk of a
  // sprite whose chunks hand the parity on -- see coverage_batch2 -- and a toggle left of the window is in that parity already.)
  const int t = rd - xb + 1;
  const bool tog = act && !dup && t < npx && (left_acts || t >= 0);
  const int tc = min(max(t, 0), npx - 1);
  atomicXor(Tcol + (tc >> 5) * SWB_WAVE, tog ? (1u << (tc & 31)) : 0u);
  // crossing pixels [ROUND_UP, ROUND_DOWN]: one pixel, or none when a non-negative crossing sits on a half.  (For
  // x >= 0 two distinct pixels, ROUND_UP < ROUND_DOWN, cannot occur: rounding x + 0.5 and x - 0.5 to float32 only
  // moves floor(x + 0.5) up and ceil(x - 0.5) down, and in exact arithmetic ceil(x - 0.5) <= floor(x + 0.5).)
  const int pu = ru - xb;
  const bool oku = act && ru <= rd && (uint32_t)pu < (uint32_t)npx;
  const int puc = min(max(pu, 0), npx - 1);
  atomicOr(Pcol + (puc >> 5) * SWB_WAVE, oku ? (1u << (puc & 31)) : 0u);
}

template <int NW>
__device__ __forceinline__ void coverage_batch2(const swb_params& p, wave_lds<NW>* L, const edge_rec* edges, uint32_t* spans,
                                                int32_t* ovf, int nspr, int yb, int sp_ymin, int sp_ymax, uint32_t sp_a,
                                                int sp_e0, row_spans& rs, uint32_t& err) {
  constexpr int NWA = SWB_NWA(NW);
  const int l = lane_id();
  const int y = yb + l;
  const uint32_t last_mask = (p.Wc & 31) ? ((1u << (p.Wc & 31)) - 1u) : 0xffffffffu;
  const int last_w = (p.Wc - 1) >> 5;
  // (the pixels beyond the canvas' last column are "covered" from the start and so never visible: no per-word clip in the word
  // loop, whose two wave-uniform conditionals per word cost three loop-invariant -- and spilled -- scalars per word)
  uint32_t covered[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) covered[w] = (w < last_w) ? 0u : ((w == last_w) ? ~last_mask : 0xffffffffu);
  rs.cnt = 0; rs.s0 = rs.s1 = rs.s2 = 0u;
  // sprites whose scan range meets this batch, front to back
  unsigned long long sm = __ballot(l < nspr && sp_ymax >= yb && sp_ymin <= yb + 63);
  while (sm) {
    const int s = 63 - __builtin_clzll(sm);
    sm &= ~(1ull << s);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)sp_a, s);
    const uint32_t e0m = (uint32_t)__builtin_amdgcn_readlane(sp_e0, s);      // first edge slot | ceil(2^16 / G) << 12
    const int e0 = (int)(e0m & 0xfffu);
    const int symin = __builtin_amdgcn_readlane(sp_ymin, s), symax = __builtin_amdgcn_readlane(sp_ymax, s);
    const int w0 = a & 31, w1 = (a >> 5) & 31, ne = (a >> 10) & 127, mer = (a >> 17) & 127, G = (int)(a >> 24);
    uint32_t prev_msb = 0u;    // last visible bit of the previous word
    int open_start = -1;
    const uint32_t sprite_bits = (uint32_t)s << 20;
    // Lane mapping of the scatter, third form ("active edges"): the two forms below give lanes to every edge of the sprite and
    // walk max(rows of an edge) rows with all of them -- but in a batch of 64 rows most edges of a big sprite have no row at all
    // (a 30-gon of 150 canvas rows: 13 of its 30 edges; a 5-pointed star of 250 rows: 4 .. 6 of 10), and a 12-sprite scene at
    // 128x128 spent two thirds of the kernel's vector instructions on lanes without a crossing (465 iterations of 64 lanes per
    // environment for about 4 500 crossings, tools/emu_stats.py).  Here the edges that DO have rows in this batch are ranked
    // (ballot + prefix count), their indices compacted through 64 dwords of LDS, and every one gets G = 2^k <= 64 / active lanes
    // that walk ITS rows in the batch with stride G: ceil(longest such edge / G) iterations.  Costs about 45 vector instructions
    // and two LDS round trips of set-up per pass, so it is tried only where the plain forms need SWB_AES_MIN_ITERS iterations or
    // more, and taken only where it saves at least two.  (Which lane visits a crossing changes nothing: the masks are built by
    // commutative LDS xor / or.)
    const bool edge_lane_form = min(mer, 64) <= ne * G;
    const int bound_all = min(min(mer, 64), min(symax, yb + 63) - max(symin, yb) + 1);
    bool packed = false;
    int pk_longest = 0;
    bool pk_hlines = false, pk_live = false;           // lane e: edge e of the sprite has rows in this batch
    int pk_xlo = 0, pk_xhi = 0;                        // ... and its crossings, toggles and crossing pixels lie in [pk_xlo, pk_xhi]
    uint32_t* const pk_slot = L->outrow;               // [64] edge index of the r-th active edge (idle P1b scratch)
    // (built into the kernels of canvases wider than 320 px only: on the 64-px .. 320-px canvases sprites rarely span more than a
    // batch or two, the form is hardly ever taken, and its mere presence cost the cover kernel 2 % there -- 11 more spilled
    // scalars, measured on 5 sprites at 64x64, anti_aliasing 5 and 1, profiles/r06_active_edges_ab.txt)
    // Sprites wider than the mask window (NWA words: every second pass of the 12-sprite scene) are scanned in x-chunks.  The
    // plain forms scatter EVERY crossing once per chunk (one left of the window toggles the window's first pixel).  Here the
    // chunks hand the parity on instead (kChain: `carry` below lives across the chunks of a pass), so that a chunk needs only
    // the edges that reach into its window: ranked and compacted per chunk, a wide sprite's left edges share the 64 lanes in its
    // first chunk and its right edges in the second.
    constexpr bool kChain = NW > SWB_AES_MAX_NARROW_NW;
    if (NW > SWB_AES_MAX_NARROW_NW && (edge_lane_form ? bound_all > (SWB_AES_MIN_ITERS - 1) * G : ne >= SWB_AES_MIN_ITERS)) {
      const bool have = l < ne;
      edge_rec ed;
      ed.x0 = ed.y0 = ed.y1 = 0; ed.dx = 0.f; ed.xtop = ed.xbot = SWB_NO_REPL; ed.pad = 0;
      if (have) ed = edges[e0 + l];
      const bool horiz = ed.y0 == ed.y1;
      const int eymin = min(ed.y0, ed.y1), eymax = max(ed.y0, ed.y1);
      const int ylo = max(max(eymin, yb), symin), yhi = min(min(eymax, yb + 63), symax);
      pk_live = have && !horiz && ylo <= yhi;
      const int na_all = __popcll(__ballot(pk_live));
      int m = pk_live ? yhi - ylo + 1 : 0;                                // longest active edge, in rows of this batch
      m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x111, 0xf, 0xf, false));   // row_shr:1
      m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x112, 0xf, 0xf, false));   // row_shr:2
      m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x114, 0xf, 0xf, false));   // row_shr:4
      m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x118, 0xf, 0xf, false));   // row_shr:8
      pk_longest = max(max(__builtin_amdgcn_readlane(m, 15), __builtin_amdgcn_readlane(m, 31)),
                       max(__builtin_amdgcn_readlane(m, 47), __builtin_amdgcn_readlane(m, 63)));
      const int lg_all = 6 - (na_all > 1 ? 32 - __clz(na_all - 1) : 0);
      const int iters_all = (pk_longest + (1 << lg_all) - 1) >> lg_all;
      // (plain edge-lane form: ceil(bound_all / G) iterations > k  <=>  bound_all > k * G)
      packed = edge_lane_form ? (iters_all + 1) * G < bound_all : iters_all + 1 < ne;
      if (packed) {
        pk_hlines = __ballot(have && horiz && ed.y0 >= yb && ed.y0 <= yb + 63 && ed.y0 < p.Hc) != 0ull;
        // x range of everything the edge can put into the masks: its crossings lie between its end points (the far one
        // recomputed from the slope: the record does not hold it), a corner replacement where its integer says; rounding, the
        // toggle one pixel right of a crossing and float32 slack are in the margins (those of sprite_rec::w0 / w1)
        const float x1f = pil_cross(ed.y1, ed.y0, ed.dx, ed.x0);
        int xlo = min((int)ed.x0, (int)floorf(x1f)), xhi = max((int)ed.x0, (int)ceilf(x1f));
        if (ed.xtop != SWB_NO_REPL) { xlo = min(xlo, (int)ed.xtop); xhi = max(xhi, (int)ed.xtop); }
        if (ed.xbot != SWB_NO_REPL) { xlo = min(xlo, (int)ed.xbot); xhi = max(xhi, (int)ed.xbot); }
        pk_xlo = xlo - 3; pk_xhi = xhi + 4;
      }
    }
    uint32_t carry = 0u;       // parity carried into the next word (all-ones or zero)
    for (int wc = w0; wc <= w1; wc += NWA) {          // x-chunks of NWA words (one for most sprites)
      const int nwords = min(NWA, w1 - wc + 1);
      const int xb = 32 * wc, npx = 32 * nwords;
      const bool left_acts = !kChain || wc == w0;      // (see scatter_crossing2)
      if (!kChain) carry = 0u;
      if (packed) {
        // the edges of this chunk: ranked, their indices compacted, G = 2^lg lanes each
        const bool in_chunk = pk_live && pk_xlo < xb + npx && (left_acts || pk_xhi >= xb);
        const unsigned long long am = __ballot(in_chunk);
        const int pk_na = __popcll(am);
        const int pk_lg = 6 - (pk_na > 1 ? 32 - __clz(pk_na - 1) : 0);       // G * active <= 64
        const int pk_iters = pk_na ? (pk_longest + (1 << pk_lg) - 1) >> pk_lg : 0;
        if (in_chunk) pk_slot[__popcll(am & ((1ull << l) - 1ull))] = (uint32_t)l;
        wave_sync();
        if (pk_hlines) {                                 // lanes = edges: the horizontal ones of this batch
          edge_rec eh;
          eh.x0 = eh.y0 = 0; eh.y1 = 1; eh.dx = 0.f; eh.xtop = eh.xbot = SWB_NO_REPL; eh.pad = 0;
          if (l < ne) eh = edges[e0 + l];
          if (eh.y0 == eh.y1 && eh.y0 >= yb && eh.y0 <= yb + 63 && eh.y0 < p.Hc) {
            const int x1 = __float_as_int(eh.dx);
            scatter_hline<NW>(L, xb, npx, eh.y0 - yb, min((int)eh.x0, x1), max((int)eh.x0, x1));
          }
        }
        if (pk_iters > 0) {
          const int ar = l >> pk_lg, j0 = l & ((1 << pk_lg) - 1);
          const bool have = ar < pk_na;
          edge_rec ed;
          ed.x0 = ed.y0 = ed.y1 = 0; ed.dx = 0.f; ed.xtop = ed.xbot = SWB_NO_REPL; ed.pad = 0;
          if (have) ed = edges[e0 + (int)pk_slot[ar]];
          const int eymin = min(ed.y0, ed.y1), eymax = max(ed.y0, ed.y1);
          const int ylo = max(max(eymin, yb), symin) + j0, yhi = min(min(eymax, yb + 63), symax);
          const float x0f = (float)ed.x0, xtop = repl_to_float(ed.xtop), xbot = repl_to_float(ed.xbot);
          const bool any_repl = __ballot(have && (xtop == xtop || xbot == xbot)) != 0ull;
          if (!any_repl && w0 != 0) {
            for (int j = 0; j < pk_iters; ++j) {
              const int yy = ylo + (j << pk_lg);
              scatter_crossing2<NW>(L, xb, npx, (yy - yb) & 63, have && yy <= yhi, yy, x0f, ed.y0, ed.dx, xtop, xbot, false, false,
                                    eymin, eymax, symax, left_acts);
            }
          } else {
            for (int j = 0; j < pk_iters; ++j) {
              const int yy = ylo + (j << pk_lg);
              scatter_crossing2<NW>(L, xb, npx, (yy - yb) & 63, have && yy <= yhi, yy, x0f, ed.y0, ed.dx, xtop, xbot, any_repl, w0 == 0,
                                    eymin, eymax, symax, left_acts);
            }
          }
        }
      } else
      // Lane mapping of the scatter.  Edge-lane form: every edge gets G = 64 / n_edges lanes that walk its rows in this batch
      // with stride G -- ceil(rows / G) iterations for ALL edges at once; row-lane form: lanes = canvas rows, one iteration per
      // edge.  The first is taken whenever it needs no more iterations than the second (round 4: it was reserved for shapes
      // whose longest edge has fewer rows than they have edges, i.e. the 30-gons; squares, tiny sprites and stars gain).
      if (min(mer, 64) <= ne * G) {
        const int e = (int)(((uint32_t)l * (e0m >> 12)) >> 16), j0 = l - e * G;                  // l / G, l % G (exact: see sp_e0)
        const bool have = e < ne;
        edge_rec ed;
        ed.x0 = ed.y0 = ed.y1 = 0; ed.dx = 0.f; ed.xtop = ed.xbot = SWB_NO_REPL; ed.pad = 0;
        if (have) ed = edges[e0 + e];
        const bool horiz = ed.y0 == ed.y1;
        const int eymin = min(ed.y0, ed.y1), eymax = max(ed.y0, ed.y1);
        if (have && horiz && j0 == 0) {
          if (ed.y0 >= yb && ed.y0 <= yb + 63 && ed.y0 < p.Hc) {
            const int x1 = __float_as_int(ed.dx);
            scatter_hline<NW>(L, xb, npx, ed.y0 - yb, min((int)ed.x0, x1), max((int)ed.x0, x1));
          }
        }
        const int ylo = max(max(eymin, yb), symin), yhi = min(min(eymax, yb + 63), symax);
        const bool live = have && !horiz && ylo <= yhi;
        const float x0f = (float)ed.x0, xtop = repl_to_float(ed.xtop), xbot = repl_to_float(ed.xbot);
        const bool any_repl = __ballot(live && (xtop == xtop || xbot == xbot)) != 0ull;
        // (rows any edge can have in this batch: its own, and those of the sprite's scan range that lie in the batch)
        const int bound = min(min(mer, 64), min(symax, yb + 63) - max(symin, yb) + 1);
        // (unswitched on the two pass-level flags: a sprite without corner replacements that does not reach the canvas' first
        // word -- the common case -- runs a loop with a straight-line body; the general loop compiles to four or five branches per
        // iteration, and on the critical path of a wave a taken branch costs more than the arithmetic around it: -1.5 % at 8192
        // environments, -2.4 % at 1024, measured twice in round 4)
        if (!any_repl && w0 != 0) {
          for (int j = 0; j < bound; j += G) {
            const int yy = ylo + j0 + j;
            scatter_crossing2<NW>(L, xb, npx, (yy - yb) & 63, live && yy <= yhi, yy, x0f, ed.y0, ed.dx, xtop, xbot, false, false,
                                  eymin, eymax, symax, left_acts);
          }
        } else {
          for (int j = 0; j < bound; j += G) {
            const int yy = ylo + j0 + j;
            scatter_crossing2<NW>(L, xb, npx, (yy - yb) & 63, live && yy <= yhi, yy, x0f, ed.y0, ed.dx, xtop, xbot, any_repl, w0 == 0,
                                  eymin, eymax, symax, left_acts);
          }
        }
      } else {
        // few long edges: lanes = canvas rows, uniform loop over the edges
        // (fetching all records of the sprite up front, lane e = edge e, and reading them back with v_readlane was
        // measured: no gain at 5 sprites, 4 % slower at 12 -- the LDS broadcast read is cheap, the readlanes are not)
        for (int e = 0; e < ne; ++e) {
          const edge_rec ed = edges[e0 + e];
          const int x0 = rfl(ed.x0), y0 = rfl(ed.y0), y1 = rfl(ed.y1);
          const float dx = rflf(ed.dx);
          if (y0 == y1) {
            if (y0 < yb || y0 > yb + 63) continue;
            const int x1 = __float_as_int(dx);
            if (y == y0) scatter_hline<NW>(L, xb, npx, l, min(x0, x1), max(x0, x1));
            continue;
          }
          const int eymin = min(y0, y1), eymax = max(y0, y1);
          if (eymax < yb || eymin > yb + 63) continue;
          const int it = rfl(ed.xtop), ib = rfl(ed.xbot);
          const bool act = (y >= eymin) && (y <= eymax) && (y >= symin) && (y <= symax);
          scatter_crossing2<NW>(L, xb, npx, l, act, y, (float)x0, y0, dx, repl_to_float(it), repl_to_float(ib),
                                it != SWB_NO_REPL || ib != SWB_NO_REPL, w0 == 0, eymin, eymax, symax, left_acts);
        }
      }
      // masks -> coverage -> visible spans
      const uint32_t wbits = ((1u << nwords) - 1u) << wc;      // canvas words of this chunk
      wave_sync();
      // (covered[] lives in registers, so the loop is unrolled over every canvas word; wide canvases skip the
      // words outside the chunk SWB_WORD_GROUPS at a time)
      constexpr int WG = NW > 5 ? SWB_WORD_GROUPS : 1;
#pragma clang loop unroll(full)
      for (int wg = 0; wg < NW; wg += WG) {
      if (WG > 1 && !((wbits >> wg) & ((1u << WG) - 1u))) continue;
#pragma clang loop unroll(full)
      for (int w = wg; w < wg + WG && w < NW; ++w) {
        if (!((wbits >> w) & 1u)) continue;         // uniform: not in this chunk
        uint32_t t = atomicExch(&L->T[w - wc][l], 0u);          // read and clear in one LDS operation (ds_wrxchg_rtn_b32)
        const uint32_t px = atomicExch(&L->Px[w - wc][l], 0u);
        // inclusive prefix xor over bits: bit b = xor of toggle bits <= b
        t ^= t << 1; t ^= t << 2; t ^= t << 4; t ^= t << 8; t ^= t << 16;
        t ^= carry;
        carry = (uint32_t)((int32_t)t >> 31);
        const uint32_t cov = t | px;
        const uint32_t vis = cov & ~covered[w];
        covered[w] |= cov;
        uint32_t d = vis ^ ((vis << 1) | prev_msb);   // transitions
        prev_msb = vis >> 31;
        // a row rarely has more than two transitions in one word: two straight-line steps, then the loop
        auto take = [&]() __attribute__((always_inline)) {      // one divergent region: the lanes that close a run
          const bool has = d != 0u;
          const int pos = 32 * w + (__ffs(d) - 1);
          d &= d - 1u;                                          // (0 stays 0)
          if (has && open_start >= 0)
            put_span(p, spans, ovf, rs, l, (uint32_t)open_start | ((uint32_t)pos << 10) | sprite_bits, err);
          open_start = has ? (open_start < 0 ? pos : -1) : open_start;
        };
        if (__ballot(d != 0u)) {
          take();
          while (__ballot(d != 0u)) take();
        }
      }
      }
      wave_sync();
    }
    if (open_start >= 0) {   // run reaches the end of the last word the sprite touches
      put_span(p, spans, ovf, rs, l, (uint32_t)open_start | ((uint32_t)(32 * (w1 + 1)) << 10) | sprite_bits, err);
    }
  }
  rs.cnt = min(rs.cnt, (uint32_t)(SWB_REG_SPANS + p.span_cap + p.ovf_cap));
  wave_sync();
}

// Median of three (= clamp of a wave-uniform x to a per-lane [lo, hi], lo <= hi) in one VALU op.
__device__ __forceinline__ int med3_su(int x_uniform, int lo, int hi) {
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "s"(x_uniform), "v"(lo), "v"(hi));
  return r;
}

// clip8 of Pillow Resample.c: (2^21 + sum) >> 22 clamped to [0,255].  The rounding constant
// 2^21 is folded into the accumulators' initial value (SWB_HALF).
#define SWB_HALF (1 << (PRECISION_BITS - 1))
__device__ __forceinline__ int clip8_fix(int acc_plus_half) {
  return min(max(acc_plus_half >> PRECISION_BITS, 0), 255);
}

// --------------------------------------------------------------------------------------------
// Hand-off between the two kernels of a step (layout: see swb_params::runs).
// --------------------------------------------------------------------------------------------
#define SWB_COST_BUCKETS 32
#define SWB_COST_SHARDS 8
// The i-th task of shard `sh` in order of decreasing cost (bucket), from the bucket counts of set `par`; -1 when fewer were
// filed.  Lanes = buckets (lane k: bucket 31 - k): one vector load, a prefix sum over the lanes, a ballot -- two memory round
// trips in all.  (Walking the buckets with one scalar load each was 32 DEPENDENT round trips at the head of every wave of
// the launch, all to the same two cache lines: the wave timeline showed a quarter of the waves beginning their lists 9-23 us
// after the launch.)
#define SWB_COST_SET (SWB_COST_SHARDS * SWB_COST_BUCKETS)
__device__ __forceinline__ int cost_row0(int par, int sh) { return (par * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS; }
__device__ __forceinline__ int cost_row1(int ph, int sh) { return 2 * SWB_COST_SET + (ph * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS; }
// words behind the counters: log2 of a priority level of the resample waves (bytes of list); per set of kind 1 the log2 of the
// bucket width its cycle counts were filed with; per launch phase the log2 of a priority level of its cover waves (cycles).
// Every word a wave reads when it begins was written by an EARLIER launch (no race with this launch's housekeeping).
#define SWB_COST_WORD_COVER_SHIFT(ph) (5 * SWB_COST_SET + 1 + (ph))
#define SWB_COST_WORD_COVER_PRIO(ph) (5 * SWB_COST_SET + 4 + (ph))
#define SWB_COST_WORD_PRIO_SHIFT(par) (5 * SWB_COST_SET + 7 + (par))      // read by the launch of parity `par`, written by the one before
#define SWB_COST_WORD_COVER_MAX(ph, sh) (5 * SWB_COST_SET + 9 + (ph) * SWB_COST_SHARDS + (sh))   // longest cycle count among the waves beyond the top bucket
// The key of a task of the resample / fill kernel is the COST of its run list: SWB_RUN_COST per run + SWB_UNIT_COST per 8-byte unit
// of the list (a unit = a run's first span, each further pair of spans another) -- the kernel's vector instructions to within a
// constant factor: 25 per run + 8 per span; the wave timeline of the headline scene, SIMD end times regressed on the runs and spans
// of their eight tasks, gives the same ratio (profiles/r05_dispatch_balance.md).  The list's length alone, the key until round 5 and
// in 8 .. 10 coarse buckets, charges a two-span run twice a one-span run: the eight tasks of a SIMD then differed by 3.0 % (one
// sigma) / 9 % (worst SIMD) in true work, and a launch ends with its slowest SIMD; by cost in fitted buckets: 1.0 % / 3 % (measured).
// bucket = ((cost - lo) * scale) >> 16 clamped to [0, 31]: lo and scale = (30 << 16) / range are fitted by every launch's second
// kernel to the costs it saw (the histogram between its 64th-part tails) for the NEXT launch -- a word per parity, read by the launch
// of that parity, written by the one before.  (5 per run + 2 per span counted with four ballots balances the headline scene a
// little better still, but mis-orders scenes of many spans per row -- spans beyond a run's third are not in it -- and costs the cover
// kernel more than it gains the second: -0.9 % / +0.9 % per step on 5 / 12 sprites against -0.5 % / +-0 for this form.)
#define SWB_COST_WORD_KEY_LO(par) (5 * SWB_COST_SET + 9 + 3 * SWB_COST_SHARDS + (par))
#define SWB_COST_WORD_KEY_RANGE(par) (5 * SWB_COST_SET + 11 + 3 * SWB_COST_SHARDS + (par))
#define SWB_COST_WORD_KEY_SCALE(par) (5 * SWB_COST_SET + 13 + 3 * SWB_COST_SHARDS + (par))
// Split bands (swb_params::split_bands): the decision word of the launch of parity `par` (1: an environment that resamples or
// fills files its band tasks; 0: one whole task), written by the launch before it, and the frames that launch's cover waves
// filed to resample or fill: a set of counters per parity, laid out and cleared like the kind-0 buckets, 32 per shard -- an
// environment counts in word (environment / 8) % 32 of its shard.  (One word per shard was measured first: on `embodied_s12`,
// where 94 % of the waves build, 7 700 atomics on eight words made the cover kernel 15 % longer.)
#define SWB_COST_WORD_SPLIT(par) (5 * SWB_COST_SET + 15 + 3 * SWB_COST_SHARDS + (par))
#define SWB_COST_WORD_SPLIT_CNT(par, sh, k) (5 * SWB_COST_SET + 17 + 3 * SWB_COST_SHARDS + ((par) * SWB_COST_SHARDS + (sh)) * SWB_COST_BUCKETS + (k))
#define SWB_COST_WORDS (17 + 3 * SWB_COST_SHARDS + 2 * SWB_COST_SET)
// A task word of the second kernel: environment | column group << 24 | band << 26 (swb_params::band_tasks) | SWB_TASK_WHOLE
#define SWB_TASK_WHOLE (1 << 29)
#define SWB_RUN_COST 3
#define SWB_UNIT_COST 2
#define SWB_KEY_BUCKETS_FITTED 30          // of the 32: one bucket of slack at either end
__device__ __forceinline__ uint32_t key_scale(uint32_t range) { return (uint32_t)(((unsigned long long)SWB_KEY_BUCKETS_FITTED << 16) / max(range, 1u)); }
__device__ __forceinline__ int cost_key(int cost, uint32_t lo, uint32_t scale) {
  const unsigned long long d = (unsigned long long)(uint32_t)max(cost - (int)lo, 0) * scale;
  return (int)min(d >> 16, (unsigned long long)(SWB_COST_BUCKETS - 1));
}
// cnt: the 32 counts of a shard (bucket 0 first); list: its 32 lists of `cap` entries
__device__ __forceinline__ int cost_ordered_entry(const uint32_t* cnt, cptr<int32_t> list, int cap, int i, int* bucket = nullptr, int* filed = nullptr) {
  static_assert(SWB_COST_BUCKETS == 32, "lanes 0..31 = buckets");
  const int l = lane_id();
  const int c = (l < SWB_COST_BUCKETS) ? (int)cnt[SWB_COST_BUCKETS - 1 - l] : 0;
  int incl = c;                                                           // inclusive prefix sum, heaviest bucket first
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);   // row_shr:1
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);   // row_shr:2
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);   // row_shr:4
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);   // row_shr:8
  const int first_row = __builtin_amdgcn_readlane(incl, 15);
  incl += (l >= 16) ? first_row : 0;
  if (filed) *filed = __builtin_amdgcn_readlane(incl, SWB_COST_BUCKETS - 1);     // entries of the shard in all
  const unsigned long long hit = __ballot(l < SWB_COST_BUCKETS && i < incl);
  if (hit == 0ull) return -1;
  const int f = __builtin_ctzll(hit);                                     // the first bucket whose running count exceeds i
  const int before = __builtin_amdgcn_readlane(incl, f) - __builtin_amdgcn_readlane(c, f);
  if (bucket) *bucket = SWB_COST_BUCKETS - 1 - f;
  return list[(size_t)rfl(SWB_COST_BUCKETS - 1 - f) * cap + rfl(i - before)];
}
// ... of the resample / fill kernel's tasks
__device__ __forceinline__ int cost_ordered_env(const swb_params& p, int par, int sh, int i, int* filed = nullptr) {
  return cost_ordered_entry(p.cost_cnt + cost_row0(par, sh), as_const(p.cost_list) + (size_t)(par * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS * p.cost_cap,
                            p.cost_cap, i, nullptr, filed);
}
__device__ __forceinline__ uint32_t log2_level(uint32_t mean, int div) { return (uint32_t)max(31 - __clz((int)max(mean / (uint32_t)max(div, 1), 2u)), 4); }
// The second kernel of a launch clears the kind-0 counters the NEXT launch files into (idle now) and derives, from the complete
// histogram of this launch's tasks, the buckets the NEXT launch files with (SWB_COST_WORD_KEY_*) and the width of a priority
// level of the next launch's resample waves (a word per parity: no wave of this launch reads a word this launch writes).
__device__ __forceinline__ void cost_housekeeping(const swb_params& p, int shard_block, int wave) {
  const int l = lane_id();
  if (shard_block < SWB_COST_SHARDS && wave == 0 && l < SWB_COST_BUCKETS) p.cost_cnt[cost_row0(p.parity ^ 1, shard_block) + l] = 0u;
  if (p.split_bands && shard_block < SWB_COST_SHARDS && wave == 0 && l < SWB_COST_BUCKETS) p.cost_cnt[SWB_COST_WORD_SPLIT_CNT(p.parity ^ 1, shard_block, l)] = 0u;
  if (shard_block == 0 && wave == 1) {
    // split bands: the next launch splits when this one's cover waves filed at most split_when frames to resample or fill (complete:
    // a kernel boundary lies behind them); a launch on a state view hands on the word it was given
    if (p.split_bands) {
      int frames = 0;
      if (l < SWB_COST_BUCKETS)
        for (int sh = 0; sh < SWB_COST_SHARDS; ++sh) frames += (int)p.cost_cnt[SWB_COST_WORD_SPLIT_CNT(p.parity, sh, l)];
      for (int o = 16; o > 0; o >>= 1) frames += __shfl_xor(frames, o, 64);
      if (l == 0) p.cost_cnt[SWB_COST_WORD_SPLIT(p.parity ^ 1)] = p.split_carry ? p.cost_cnt[SWB_COST_WORD_SPLIT(p.parity)] : ((p.split_when > 0 && frames <= p.split_when) ? 1u : 0u);
    }
    int c = 0;
    if (l < SWB_COST_BUCKETS)
      for (int sh = 0; sh < SWB_COST_SHARDS; ++sh) c += (int)p.cost_cnt[cost_row0(p.parity, sh) + l];
    int n0 = c, s0 = c * (2 * l + 1);                                    // (bucket centre, in half buckets)
    for (int o = 16; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); n0 += __shfl_xor(n0, o, 64); }
    int incl = c;                                                        // tasks in buckets 0 .. l
    for (int o = 1; o < SWB_COST_BUCKETS; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (l >= o) incl += t; }
    const int tail = max(n0 >> 6, 1);                                    // a 64th of the tasks at either end may share the end buckets
    const unsigned long long reached = __ballot(l < SWB_COST_BUCKETS && incl >= tail), below_top = __ballot(l < SWB_COST_BUCKETS && incl <= n0 - tail);
    const int c_first = __builtin_amdgcn_readlane(c, 0), c_last = __builtin_amdgcn_readlane(c, SWB_COST_BUCKETS - 1);
    if (l == 0 && n0 > 0) {
      const uint32_t lo = p.cost_cnt[SWB_COST_WORD_KEY_LO(p.parity)], range = max(p.cost_cnt[SWB_COST_WORD_KEY_RANGE(p.parity)], (uint32_t)SWB_KEY_BUCKETS_FITTED);
      // bucket k of this launch held costs [lo + k * range / 30, lo + (k + 1) * range / 30); bucket 0 also everything below, 31 everything above
      uint32_t new_lo = lo, new_range = range;
      if (c_last > (n0 >> 3)) new_range = range * 2;                                                   // the range ended too low: double it upwards
      else if (c_first > (n0 >> 3) && lo > 0) { new_lo = lo > range ? lo - range : 0u; new_range = range + (lo - new_lo); }   // ... began too high: extend it downwards
      else {
        const int b_lo = reached ? __builtin_ctzll(reached) : 0;                                        // the buckets between the two tails
        const int b_hi = below_top ? min(64 - __builtin_clzll(below_top), SWB_COST_BUCKETS - 1) : b_lo;
        const uint32_t a = lo + (uint32_t)(((unsigned long long)b_lo * range) / SWB_KEY_BUCKETS_FITTED);
        const uint32_t b = lo + (uint32_t)(((unsigned long long)(max(b_hi, b_lo) + 1) * range) / SWB_KEY_BUCKETS_FITTED);
        new_range = max(b - a, (uint32_t)SWB_KEY_BUCKETS_FITTED);
        new_lo = a > new_range / SWB_KEY_BUCKETS_FITTED ? a - new_range / SWB_KEY_BUCKETS_FITTED : 0u;          // (a bucket of slack below: costs drift)
      }
      p.cost_cnt[SWB_COST_WORD_KEY_LO(p.parity ^ 1)] = new_lo;
      p.cost_cnt[SWB_COST_WORD_KEY_RANGE(p.parity ^ 1)] = new_range;
      p.cost_cnt[SWB_COST_WORD_KEY_SCALE(p.parity ^ 1)] = key_scale(new_range);
      // mean cost -> mean list in bytes (a unit is 8 bytes and costs 2 + its share of a run's 3: about 2 bytes of list per unit of
      // cost; a level is a power of two)
      const uint32_t mean_cost = lo + (uint32_t)(((long long)s0 * range) / (2ll * SWB_KEY_BUCKETS_FITTED * n0));
      p.cost_cnt[SWB_COST_WORD_PRIO_SHIFT(p.parity ^ 1)] = (p.prio_levels & 1) ? log2_level(2u * mean_cost, p.prio_div) : 0u;
    }
  }
}
// The cover kernel keeps its own lists (kind 1) itself -- a launch may have no second kernel (anti_aliasing = 1 paints in the
// cover kernel): blocks 0..7 clear the set the NEXT launch files into (read by the previous launch, idle now); block 0 derives,
// from the complete histogram of the PREVIOUS launch, the bucket width the NEXT launch files with and the priority level of the
// next launch's waves.  No wave reads a word that a block of its own launch writes (the L2 is per XCD: a wave on another XCD
// could see either value).  The width moves in ONE step to where the heaviest environments land in the upper half of the 32
// buckets: when the top bucket overflowed (it may hold the heaviest sixteenth) to the width that fits the longest cycle count
// among the waves beyond it (a sharded maximum those waves keep); log2(16 / (highest bucket used + 1)) narrower when
// everything fitted in the lower third.  Launches 0 and 1 file with the initial 2^12 cycles, launch 2 with the right width
// (measured before, one step of +-1 per launch: 12 sprites at 128x128 needed 2^16 and reached it -- and its order -- at launch 7).
// `block`: the workgroup's index among the launch's state workgroups (the cover kernel's grid may hold copy workgroups as well).
__device__ __forceinline__ void cover_cost_housekeeping(const swb_params& p, uint32_t block, int prev, int cur, int next) {
  const int l = lane_id();
  if (block < SWB_COST_SHARDS && l < SWB_COST_BUCKETS) p.cost_cnt[cost_row1(next, (int)block) + l] = 0u;
  if (block < SWB_COST_SHARDS && l == 0) p.cost_cnt[SWB_COST_WORD_COVER_MAX(next, (int)block)] = 0u;
  if (block == 0) {
    int c = 0;
    if (l < SWB_COST_BUCKETS)
      for (int sh = 0; sh < SWB_COST_SHARDS; ++sh) c += (int)p.cost_cnt[cost_row1(prev, sh) + l];
    const int longest = wave_max_i(l < SWB_COST_SHARDS ? (int)min(p.cost_cnt[SWB_COST_WORD_COVER_MAX(prev, l)], 0x7fffffffu) : 0);
    const unsigned long long used = __ballot(c > 0);
    const int top = __builtin_amdgcn_readlane(c, SWB_COST_BUCKETS - 1);
    int n1 = c, s1 = c * (2 * l + 1);
    for (int o = 16; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); n1 += __shfl_xor(n1, o, 64); }
    if (l == 0) {
      const uint32_t width_prev = p.cost_cnt[SWB_COST_WORD_COVER_SHIFT(prev)];       // what the previous launch filed with
      uint32_t width = p.cost_cnt[SWB_COST_WORD_COVER_SHIFT(cur)], level = p.cost_cnt[SWB_COST_WORD_COVER_PRIO(cur)];
      if (used) {
        const int hi = 63 - __builtin_clzll(used);
        width = width_prev;
        if (top > (p.N >> 4)) width = (uint32_t)min(max(27 - __clz(max(longest, 1)), (int)width_prev + 1), 26);   // longest >> width in [16, 32)
        else if (hi < 12) width = (uint32_t)max((int)width_prev - max(31 - __clz(16 / (hi + 1)), 1), 1);
      }
      if (n1 > 0) level = log2_level((uint32_t)((((long long)s1 << width_prev) >> 1) / n1), p.prio_div);   // mean cover wave, in cycles
      p.cost_cnt[SWB_COST_WORD_COVER_SHIFT(next)] = width;
      p.cost_cnt[SWB_COST_WORD_COVER_PRIO(next)] = level;
    }
  }
}

// Which block of its shard's cost order a workgroup serves.  The dispatcher hands consecutive workgroups of an XCD to its
// compute units breadth-first (measured: workgroup b runs on XCD b % 8, and the XCD-local workgroups j and j + 32 on the same
// CU), so dealing every round of 2^deal_shift workgroups in descending order gives the first CU the heaviest block of every
// round and the last CU the lightest (measured on 8192 environments: 182 against 158 units per wave, its SIMDs done at 105 against
// 94 us).  Odd rounds are dealt in ascending order instead.
__device__ __forceinline__ int dealt_block(const swb_params& p, int j, int blocks) {
  if (p.deal_shift <= 0) return j;
  const int base = (j >> p.deal_shift) << p.deal_shift;
  if (!((j >> p.deal_shift) & 1)) return j;
  const int m = min(1 << p.deal_shift, blocks - base);      // (the last round may be short)
  return base + (m - 1 - (j - base));
}

#define SWB_MAX_CG 4                     // groups of 64 output columns (images up to 256 columns)
#define SWB_MAX_BANDS 8                  // bands of output rows
#define SWB_RHDR_GROUPS 32               // header dword of the first column-group block
#define SWB_RHDR_GSTRIDE (1 + SWB_MAX_BANDS)
// ... behind the column-group blocks: what a later launch needs to KEEP the lists (swb_params::list_epoch) -- the cost each
// group's list was filed under (the one thing the filing cannot recompute from the header), then the validity stamp: the epoch
// of the launch that built the lists, or 0 (built with an error, moved to the arena, or by a launch that keeps nothing); then
// the cycles the wave that built them took -- what a wave that keeps them files its environment under for the order of the
// next cover launch (its own few cycles would put the environment last, at the lowest priority, in the launch that has to
// build its lists again)
#define SWB_RHDR_COST (SWB_RHDR_GROUPS + SWB_MAX_CG * SWB_RHDR_GSTRIDE)
#define SWB_RHDR_STAMP (SWB_RHDR_COST + SWB_MAX_CG)
#define SWB_RHDR_CYCLES (SWB_RHDR_STAMP + 1)
// ... and the state of the environment's frame in the engine's cache (swb_params::frame_cache), written by the cover wave alone:
// 0 the cache does not hold it (the wave BUILT its lists, or the handle has no cache), 1 the resample waves of this launch
// leave it there (the first launch that kept the lists), 2 it is there: the frame is a copy of it.  A wave that keeps writes
// min(old + 1, 2).  The copy workgroups of the cover launch (swb_params::spec_copy) read the word while that wave may be writing it.
#define SWB_RHDR_FRAME (SWB_RHDR_CYCLES + 1)
// Split bands (swb_params::split_bands): the bands a changed frame is cut into.
#define SWB_SPLIT_BANDS_DEFAULT 8
#define SWB_RHDR_DWORDS (SWB_RHDR_STAMP + 4)
#define SWB_BST_STRIDE (SWB_MAX_BANDS + 1)   // band starts of a list + its end, in LDS (swb_params::band_tasks: see emit_runs)
__device__ __forceinline__ int run_units(int spans) { return spans <= 1 ? 1 : 2 + (spans > 3 ? (spans - 2) >> 1 : 0); }
// Bit 23 of a run's first dword: a CONTINUATION run (anti_aliasing > 1 only).  Its rows have the spans of the run before it in the
// list, which ended only because an output row's window ended with it; the record is one unit whatever that run's span count
// (the spans field repeats the count, at least 1; the span dword is not read).
#define SWB_RUN_CONTINUES (1u << 23)
// Pins a scalar load in front of the branches that follow it (an empty statement that "uses" the value).  Without it the compiler
// sinks the resample loop's two table loads below the test for the kind of run and joins the paths again through a flag register:
// three more scalar instructions and a second taken branch for every run.
#if defined(__HIP_DEVICE_COMPILE__)
#define SWB_LOADED_HERE(v) __asm__ volatile("" : "+s"(v))
#else
#define SWB_LOADED_HERE(v) ((void)0)
#endif
// d = a << SH | b as ONE v_lshl_or_b32 (the compiler renders the C expression of a three-byte pack as two shifts and a three-input
// or).  For the device only: the host side of the compilation, and a build of these sources for the host, take the C meaning.
#if defined(__HIP_DEVICE_COMPILE__)
#define SWB_LSHL_OR(d, a, SH, b) __asm__("v_lshl_or_b32 %0, %1, " #SH ", %2" : "=v"(d) : "v"(a), "v"(b))
#else
#define SWB_LSHL_OR(d, a, SH, b) ((d) = ((a) << (SH)) | (b))
#endif

// Hook of the profiling builds under tools/overlays (kernel cut short after a phase): nothing in the product.
#ifndef SWB_HOOK_PHASE_END
#define SWB_HOOK_PHASE_END(k)
#endif

// Span i (any i < rs.cnt) of the canvas row this lane owns in the current batch.
__device__ __forceinline__ uint32_t lane_span(const swb_params& p, const uint32_t* spans, const int32_t* ovf, const row_spans& rs,
                                              int i, int l) {
  if (i == 0) return rs.s0;
  if (i == 1) return rs.s1;
  if (i == 2) return rs.s2;
  const int k = i - SWB_REG_SPANS;
  if (k < p.span_cap) return spans[k * SWB_WAVE + l];
  const int s = *(volatile const int32_t*)ovf;
  return s >= 0 ? p.ovf[((size_t)s * 64 + l) * p.ovf_cap + (k - p.span_cap)] : 0u;
}

// The rare path of emit_runs: the list of column group g stands at position base_g (counted from the first unit of its own part),
// meta_g = next band | log2(capacity / run_cap) << 4 | (its arena segment / 32) << 8, and the batch adds `total` units.  Returns
// { position, meta } with room for them -- after MOVING the list to a segment of the arena twice (four times ...) as large when
// its current one is too small: the wave copies what it has written, shifts the band starts already recorded -- or { ~0, . }
// when the arena is exhausted.  All lanes call it; the arguments are wave-uniform.
__device__ __forceinline__ uint2 list_room_or_move(const swb_params& p, int env, int g, uint32_t* runs_env, uint32_t* hdr,
                                                             uint32_t* bst, int base_g, uint32_t meta_g, int total) {
  const int l = lane_id();
  const int seg_k = (int)((meta_g >> 4) & 15u), next_band_g = (int)(meta_g & 15u);
  const long long arena_rel = p.arena_base - ((long long)env * p.ncg + g) * p.run_cap;     // the arena's first unit, as a position of this list
  const int start_g = seg_k ? (int)(arena_rel + 32ll * (long long)(meta_g >> 8)) : 0;
  if (base_g + total < start_g + (p.run_cap << seg_k)) return make_uint2((uint32_t)base_g, meta_g);
  if (p.arena_units <= 0) return make_uint2(0xffffffffu, meta_g);
  const int pos = base_g - start_g;
  int k2 = seg_k;
  do ++k2; while (k2 < 12 && pos + total >= (p.run_cap << k2));
  const uint32_t alloc = (uint32_t)(((p.run_cap << k2) + 31) & ~31);
  uint32_t a = 0u;
  if (l == 0) a = atomicAdd(&p.arena_head[p.parity], alloc);
  a = (uint32_t)rfl((int)a);
  if (pos + total >= (p.run_cap << k2) || (unsigned long long)a + alloc > (unsigned long long)(uint32_t)p.arena_units)
    return make_uint2(0xffffffffu, meta_g);
  const int new_start = (int)(arena_rel + (long long)a);
  uint32_t* const lst = runs_env + (size_t)g * p.run_cap * 2;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");                    // (what other lanes of this wave wrote to the list and the header)
  for (int i = l; i < pos; i += SWB_WAVE)
    *reinterpret_cast<uint2*>(lst + 2 * ((long long)new_start + i)) = *reinterpret_cast<const uint2*>(lst + 2 * ((long long)start_g + i));
  if (l < next_band_g) hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE + 1 + l] += (uint32_t)(new_start - start_g);   // bands recorded so far
  if (bst && l < next_band_g) bst[g * SWB_BST_STRIDE + l] += (uint32_t)(new_start - start_g);                    // (their copy in LDS)
  return make_uint2((uint32_t)(new_start + pos), (meta_g & 15u) | ((uint32_t)k2 << 4) | ((a >> 5) << 8));
}

// --------------------------------------------------------------------------------------------
// End of P2 for one batch of 64 canvas rows: the rows' visible spans (registers + LDS lists + overflow slot of
// the lane that owns the row) become RUNS in the hand-off lists, one list per group of 64 output columns.
//   * a row whose spans equal those of the row above continues that row's run (vertical edges, flat tops: the
//     horizontal pass gives the same result and the vertical pass is linear in it), unless an output row ends
//     between them or a band of output rows starts there (swb_params::v_break);
//   * where only the end of an output row's window stands between them (anti_aliasing > 1), the row starts a CONTINUATION run: one
//     unit without spans (SWB_RUN_CONTINUES) -- the resample kernel keeps the horizontal pass of the run before it.  Never the
//     first run of a batch of 64 rows or of a band (the wave that starts at a band has no row yet); a list that moves to the
//     arena stays one contiguous array, so a continuation always follows its head;
//   * with a black background a row without spans adds nothing and is not listed (anti_aliasing = 1: never
//     listed, the fill kernel paints what no run covers with the background);
//   * images wider than 64 columns: a column group lists only the spans its resampling windows reach, clipped to
//     that range (a clipped span has the same weights), so the groups fold and skip rows independently.
// The first unit of every band (the first run at or below the band's first canvas row) goes to the header.
// --------------------------------------------------------------------------------------------
// base_l / band_l: lane g holds, for column group g, the units its list holds so far and the next band whose first unit is
// still to be recorded (wave-uniform values kept in a vector register: the loop over the groups stays a loop).
// bst (swb_params::band_tasks, else null): [ncg][SWB_BST_STRIDE] in LDS, a copy of the band starts recorded in the header -- the
// filing at the end of the kernel prices every band from them.
__device__ __forceinline__ void emit_runs(const swb_params& p, const uint32_t* spans, const int32_t* ovf, const row_spans& rs,
                                          int yb, int env, uint32_t* runs_env, uint32_t* hdr, uint32_t* bst, int& base_l, int& band_l,
                                          int& cost_l, uint32_t& err) {
  const int l = lane_id();
  const int y = yb + l;
  const bool valid = y < p.Hc;
  // break bits of rows yb .. yb + 63: three words of the (padded) table through scalar loads, picked per lane
  cptr<uint32_t> bw = as_const(p.v_break) + (yb >> 5);
  const unsigned long long b01 = (unsigned long long)bw[0] | ((unsigned long long)bw[1] << 32);
  const int bp = (yb & 31) + l;                                         // 0 .. 94
  const bool brk = ((bp < 64 ? (uint32_t)(b01 >> bp) : (bw[2] >> (bp - 64))) & 1u) != 0u;
  // ... and the same of the table behind it: rows where a band starts (no continuation run there: the band's wave has no row yet)
  bool may_continue = false;
  if (p.AA != 1) {
    cptr<uint32_t> sw = bw + (((p.Hc + 31) >> 5) + 3);
    const unsigned long long s01 = (unsigned long long)sw[0] | ((unsigned long long)sw[1] << 32);
    may_continue = brk && ((bp < 64 ? (uint32_t)(s01 >> bp) : (sw[2] >> (bp - 64))) & 1u) == 0u;
  }
  const int cnt = valid ? (int)rs.cnt : 0;
  // (the longest span list of the batch: only the slow paths below need it)
  const int maxc = (p.ncg != 1 || __ballot(cnt > SWB_REG_SPANS)) ? wave_max_i(cnt) : SWB_REG_SPANS;
  const bool list_empty_rows = p.bg != 0u && p.AA != 1;
#pragma clang loop unroll(disable)
  for (int g = 0; g < p.ncg; ++g) {
    int base_g = __builtin_amdgcn_readlane(base_l, g);
    // band_l: next band | log2(capacity / run_cap) << 4 | (the arena segment the list lives in, / 32) << 8
    uint32_t meta_g = (uint32_t)__builtin_amdgcn_readlane(band_l, g);
    int next_band_g = (int)(meta_g & 15u);
    const int lo = (p.ncg == 1) ? 0 : as_const(p.cg_lo)[g], hi = (p.ncg == 1) ? 1024 : as_const(p.cg_hi)[g];
    uint32_t f0 = rs.s0, f1 = rs.s1, f2 = rs.s2;
    int fc = cnt;
    if (p.ncg != 1) {                              // the spans this group's columns can see, clipped
      f0 = f1 = f2 = 0u; fc = 0;
      // (the three spans in registers straight-line, in lane_span's order: its switch costs a wave-uniform branch tree per span.
      // A macro, not a lambda: with the counters captured by reference the compiler left them in scratch memory.)
#define SWB_SEE_SPAN(V, HAVE)                                                                                     \
      do {                                                                                                        \
        const uint32_t v_ = (V);                                                                                  \
        const int a_ = (int)(v_ & 1023u), b_ = (int)((v_ >> 10) & 1023u);                                         \
        if ((HAVE) && a_ < hi && b_ > lo) {                                                                       \
          const uint32_t c_ = (uint32_t)max(a_, lo) | ((uint32_t)min(b_, hi) << 10) | (v_ & 0xfff00000u);         \
          if (fc == 0) f0 = c_; else if (fc == 1) f1 = c_; else if (fc == 2) f2 = c_;                             \
          ++fc;                                                                                                   \
        }                                                                                                         \
      } while (0)
      SWB_SEE_SPAN(rs.s0, 0 < cnt);
      if (maxc > 1) SWB_SEE_SPAN(rs.s1, 1 < cnt);
      if (maxc > 2) SWB_SEE_SPAN(rs.s2, 2 < cnt);
      for (int i = SWB_REG_SPANS; i < maxc; ++i) SWB_SEE_SPAN(lane_span(p, spans, ovf, rs, i, l), i < cnt);
#undef SWB_SEE_SPAN
    }
    const bool nonempty = valid && (list_empty_rows || fc > 0);
    // the row above, one lane down (wave_shr:1); a row that is not listed never compares equal
    const int pc = __builtin_amdgcn_update_dpp(-2, nonempty ? fc : -2, 0x138, 0xf, 0xf, false);
    const int p0 = __builtin_amdgcn_update_dpp(0, (int)f0, 0x138, 0xf, 0xf, false);
    const int p1 = __builtin_amdgcn_update_dpp(0, (int)f1, 0x138, 0xf, 0xf, false);
    const int p2 = __builtin_amdgcn_update_dpp(0, (int)f2, 0x138, 0xf, 0xf, false);
    const bool same = nonempty && l > 0 && fc == pc && fc <= SWB_REG_SPANS && (int)f0 == p0 && (int)f1 == p1 && (int)f2 == p2;
    const bool cont = same && !brk;
    const bool start = nonempty && !cont;
    // a run that had to end only because an output row's window ends there: the rows below it with the same spans become a
    // CONTINUATION run -- one unit without spans, the resample kernel keeps the horizontal pass of the run before
    const bool contin = same && may_continue;
    const unsigned long long contm = __ballot(cont);
    const int len = 1 + __builtin_ctzll(~((contm >> 1) >> l));          // rows of the run that starts here (bit 63 of the shifted mask is 0)
    const int units = start ? (contin ? 1 : run_units(fc)) : 0;
    // inclusive prefix sum over the lanes: within rows of 16 lanes by DPP shifts, then the three row totals
    int incl = units;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);   // row_shr:1
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);   // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);   // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);   // row_shr:8
    {
      const int r0 = __builtin_amdgcn_readlane(incl, 15), r1 = __builtin_amdgcn_readlane(incl, 31), r2 = __builtin_amdgcn_readlane(incl, 47);
      incl += (l >= 48) ? r0 + r1 + r2 : ((l >= 32) ? r0 + r1 : ((l >= 16) ? r0 : 0));
    }
    const int total = __builtin_amdgcn_readlane(incl, SWB_WAVE - 1);
    const int excl = incl - units;
    // the list lives in its own part (positions [0, run_cap): meta_g's upper bits are zero) or, after it outgrew that, in a
    // segment of the arena (list_room_or_move: the rare path)
    bool room = base_g + total < p.run_cap;                             // (one unit stays free for the sentinel)
    if ((meta_g >> 4) != 0u || (!room && p.arena_units > 0)) {          // (wave-uniform, rare)
      const uint2 moved = list_room_or_move(p, env, g, runs_env, hdr, bst, base_g, meta_g, total);
      room = moved.x != 0xffffffffu;
      if (room) { base_g = (int)moved.x; meta_g = moved.y; }
    }
    if (!room) err |= SWB_ENV_ERR_SPAN_OVERFLOW;
    uint32_t* dst = runs_env + (size_t)g * p.run_cap * 2 + 2 * ((long long)base_g + excl);
    if (start && room) {
      *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)y | ((uint32_t)(len - 1) << 16) | (contin ? SWB_RUN_CONTINUES | ((uint32_t)max(fc, 1) << 24) : (uint32_t)fc << 24), f0);
      if (fc >= 2 && !contin) *reinterpret_cast<uint2*>(dst + 2) = make_uint2(f1, f2);
    }
    if (room && __ballot(start && fc > SWB_REG_SPANS)) {                // spans beyond three: units 2, 3, ...
      int j = 0;
#define SWB_LIST_SPAN(V, HAVE)                                                                                    \
      do {                                                                                                        \
        const uint32_t v_ = (V);                                                                                  \
        const int a_ = (int)(v_ & 1023u), b_ = (int)((v_ >> 10) & 1023u);                                         \
        if ((HAVE) && a_ < hi && b_ > lo) {                                                                       \
          const uint32_t c_ = (p.ncg == 1) ? v_ : ((uint32_t)max(a_, lo) | ((uint32_t)min(b_, hi) << 10) | (v_ & 0xfff00000u)); \
          if (j >= SWB_REG_SPANS && start) dst[2 * (2 + ((j - 3) >> 1)) + ((j - 3) & 1)] = c_;                    \
          ++j;                                                                                                    \
        }                                                                                                         \
      } while (0)
      SWB_LIST_SPAN(rs.s0, 0 < cnt);                  // (the register spans straight-line, as above; maxc >= 4 here)
      SWB_LIST_SPAN(rs.s1, 1 < cnt);
      SWB_LIST_SPAN(rs.s2, 2 < cnt);
      for (int i = SWB_REG_SPANS; i < maxc; ++i) SWB_LIST_SPAN(lane_span(p, spans, ovf, rs, i, l), i < cnt);
#undef SWB_LIST_SPAN
      if (start && fc > SWB_REG_SPANS && ((fc - 3) & 1)) dst[2 * (2 + ((fc - 3) >> 1)) + 1] = 0u;
    }
    // bands whose first canvas row lies in (or before) this batch: their first unit
    while (next_band_g < p.nbands) {
      const int y0 = as_const(p.band_y0)[next_band_g];
      if (y0 > yb + 63) break;
      // (a batch that found no room wrote nothing: its bands start where the list stands -- at the sentinel, if nothing
      // follows --, never at an offset into the part that was not written)
      const int at = base_g + ((y0 <= yb || !room) ? 0 : __builtin_amdgcn_readlane(excl, (y0 - yb) & 63));
      if (l == 0) hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE + 1 + next_band_g] = (uint32_t)at;
      if (bst && l == 0) bst[g * SWB_BST_STRIDE + next_band_g] = (uint32_t)at;
      ++next_band_g;
    }
    // what the batch adds to the cost of the list (the key it is filed under)
    // (a continuation run: the vertical pass of a run, no spans -- its unit is not charged)
    const int cost_g = SWB_RUN_COST * __popcll(__ballot(start)) + SWB_UNIT_COST * (total - __popcll(__ballot(contin)));
    if (l == g) { base_l = room ? base_g + total : base_g; band_l = (int)((meta_g & ~15u) | (uint32_t)next_band_g); cost_l += room ? cost_g : 0; }
  }
}

// After the coverage of a batch: in the (virtually never met) case that a row outgrew its register + LDS
// span lists while the wave held no HBM overflow slot, take one and scan the same batch again (the
// statement `continue`s the batch loop with yb stepped back).
#define SWB_RESCAN_WITH_OVERFLOW_SLOT()                                                          \
  if (__ballot((err & SWB_INT_NEED_SLOT) != 0u)) {                                               \
    err &= ~SWB_INT_NEED_SLOT;                                                                   \
    if (rfl(*ovf) == -1) {                                                                       \
      if (l == 0) *ovf = ovf_slot_alloc(p);                                                      \
      wave_sync();                                                                               \
      if (rfl(*ovf) >= 0) { yb -= 64; continue; }                                                \
    }                                                                                            \
    err |= SWB_ENV_ERR_SPAN_OVERFLOW;                                                            \
  }

// The frame cache's mover (swb_params::frame_cache): `rows` row segments of `seg_bytes` bytes, `row_bytes` apart, from src to dst
// at the same offsets -- a wave's rectangle of the frame, which lies alike in the caller's buffer and in the cache.  Lanes take
// consecutive chunks of T (16 bytes where both sides are aligned, else a dword: the same bytes either way), BATCH of
// them loaded before the first is stored -- a copying wave does nothing else, so the loads in flight are its whole latency hiding.
template <typename T, int BATCH>
__device__ __forceinline__ void copy_frame_rect_as(const unsigned char* src, unsigned char* dst, uint32_t row_bytes, uint32_t seg_bytes, int rows) {
  const int l = lane_id();
  const int cpr = (int)(seg_bytes / (uint32_t)sizeof(T)), total = rows * cpr;      // chunks per row segment (uniform), in all
  const int step_rows = 64 / cpr, step_cols = 64 - step_rows * cpr;               // what 64 chunks further means
  int row = l / cpr, col = l - row * cpr;
  for (int base = 0; base < total; base += 64 * BATCH) {
    T v[BATCH];
    uint32_t off[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      off[j] = (uint32_t)row * row_bytes + (uint32_t)col * (uint32_t)sizeof(T);
      if (base + 64 * j + l < total) v[j] = *reinterpret_cast<const T*>(src + off[j]);
      row += step_rows; col += step_cols;
      if (col >= cpr) { col -= cpr; ++row; }
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
      if (base + 64 * j + l < total) *reinterpret_cast<T*>(dst + off[j]) = v[j];
  }
}
typedef uint32_t swb_c16 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void copy_frame_rect(const unsigned char* src, unsigned char* dst, uint32_t row_bytes, uint32_t seg_bytes, int rows, bool aligned16) {
  if (aligned16) copy_frame_rect_as<swb_c16, 6>(src, dst, row_bytes, seg_bytes, rows);
  else copy_frame_rect_as<uint32_t, 8>(src, dst, row_bytes, seg_bytes, rows);
}

// --------------------------------------------------------------------------------------------
// A COPY workgroup of the cover launch (swb_params::spec_copy; DESIGN.md section 29): copy workgroup c serves column group
// c % ncg of environment c / ncg -- the plain index, never the cost order.  It copies the whole rows of its column group from the
// frame cache to the caller's buffer if the environment's header says the cache may hold its frame (SWB_RHDR_FRAME != 0),
// BEFORE anyone knows whether the environment keeps its lists in this launch: the copies run beside the few waves that build,
// while the memory system has nothing else to do, and the resample launch is left with the frames that changed.
//
// The word is read with one plain load while the environment's own cover wave -- its only writer during the launch -- may be
// writing it: the load returns the value the previous launch left or the new one, and either is right.
//   old -> new   the cover wave      this workgroup                     why the frame is right
//   1, 2 -> 2    kept                reads 1 or 2: copies               the cache holds the frame since the launch that wrote 1; the
//                                                                       wave files no resample task: the ONE case whose frame is the copy
//   0 -> 1       kept, fill          reads 0: nothing; 1: stale bytes   the resample waves rewrite every byte, and fill the cache
//   any -> 0     built               may copy                           the resample waves rewrite every byte
// Nothing writes the cache during the cover launch, and the launch boundary orders these stores before those of the resample
// launch.  No wave waits for another: no flag, no poll, no fence.  The workgroup touches no LDS, no cost table and no dispatch
// word, and stays at priority 0.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ void spec_copy_group(const swb_params& p, uint32_t c) {
  const uint32_t env = p.ncg == 1 ? c : c / (uint32_t)p.ncg, g = c - env * (uint32_t)p.ncg;
  if (p.rhdr[(size_t)env * SWB_RHDR_DWORDS + SWB_RHDR_FRAME] == 0u) return;
  const uint32_t cycles0 = p.frame_stats ? (uint32_t)__builtin_amdgcn_s_memtime() : 0u;
  const size_t off = (size_t)env * p.Wo * p.Ho * 3 + 192u * g;
  copy_frame_rect(p.frame_cache + off, p.obs + off, 3u * (uint32_t)p.Wo, 3u * (uint32_t)min(64, p.Wo - 64 * (int)g), p.Ho, p.obs_aligned16 != 0);
  if (p.frame_stats && lane_id() == 0) {
    atomicAdd(&p.frame_stats[3], (unsigned long long)((uint32_t)__builtin_amdgcn_s_memtime() - cycles0));
    atomicAdd(&p.frame_stats[6], 1ull);
  }
}

// --------------------------------------------------------------------------------------------
// Kernel 1 of a step, "cover": P0 state, P1 geometry, P2 coverage -> run lists.  One wave = one environment.
#endif                      // SWB_SETS_PASS
// --------------------------------------------------------------------------------------------
// OV = true: the build an engine switches to once swb_set_sprite_attr has been called (environments may carry
// per-sprite overrides of shape / scale / centred path, see swb_params::ov_flag); OV = false compiles to exactly
// the kernel without that feature.
// PAINT = true: anti_aliasing = 1 and an image of up to 64 columns (the canvas fits NW = 2) -- the wave paints the frame itself,
// there is no second kernel; a build of its own so that neither kernel carries the other's copy of the coverage code.
// SETS = true (with OV = true): swb_cover_sets_kernel, the build of handles with task sets (swb_set_task_sets; DESIGN.md section
// 31) -- finish_step looks the episode's task up by its pool entry.  A kernel of its own name, instantiated in swb_wide.hip: the
// OV = false / true builds, and the code object they live in, stay byte for byte what they were before there were task sets.
// How two kernels share one body without sharing a function (which changed the plain builds' code when it was tried): this file
// includes ITSELF once more, in swb_wide.hip only, with SWB_SETS_PASS defined -- the pass compiles nothing but the two kernel
// bodies marked for it, under the names and flags of the task-set builds.
#ifdef SWB_SETS_PASS
template <int NW, bool PAINT>
__global__ void __launch_bounds__(SWB_WAVE, SWB_COVER_WAVES(NW))
swb_cover_sets_kernel(const swb_params p) {
  constexpr bool OV = true, SETS = true;
#else
template <int NW, bool OV = false, bool PAINT = false>
__global__ void __launch_bounds__(SWB_WAVE, SWB_COVER_WAVES(NW))
swb_cover_kernel(const swb_params p) {
  constexpr bool SETS = false;
#endif
  static_assert(!PAINT || NW == 2, "painting in the cover kernel: images of up to 64 columns at anti_aliasing = 1");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // The copy workgroups of a launch with a frame cache (swb_params::spec_copy, never in the painting builds): behind the N
  // state workgroups, or (tests) in front of them.  `block` is the workgroup's index among the state workgroups.
  uint32_t block = blockIdx.x;
  if constexpr (!PAINT) {
    if (p.spec_copy != 0) {
      const uint32_t ncopy = (uint32_t)p.N * (uint32_t)p.ncg;
      const uint32_t c = p.spec_copy == 2 ? block : block - (uint32_t)p.N;      // (behind: wraps above ncopy for a state workgroup)
      if (c < ncopy) { spec_copy_group(p, c); return; }
      if (p.spec_copy == 2) block -= ncopy;
    }
  }
  const int l = lane_id();
  const uint32_t cycles0 = (uint32_t)__builtin_amdgcn_s_memtime();
  // the environment of this block: its own index, or (cover_order) the next one in order of decreasing cost of the previous step
  int env = (int)block;
  // ... and, as in the resample kernel, the wave's priority follows the work it has left: the cycles it took last time (its
  // bucket) minus the cycles since it began, one level per 2^prio_q cycles (about half a mean wave), re-evaluated at the end of
  // every phase and batch.  0 cycles predicted = no priorities (plain order, or switched off).
  uint32_t predicted = 0u, prio_q = 0u;
  int prio = 0;
  const int ph = p.cphase, ph_prev = ph == 0 ? 2 : ph - 1, ph_next = ph == 2 ? 0 : ph + 1;
  // The three dispatch words the wave files its lists with at its very end (lanes 0 .. 2: the key buckets of the second
  // kernel's tasks, the bucket width of the cover cycles): loaded at the start of the wave, a round trip to memory that the end of the wave --
  // nothing behind it to hide a latency -- does not wait for.  (All three were written by an earlier launch.)
  uint32_t filing_words_l = 0u;
  // (lane 3, split bands: the launch's decision word, SWB_COST_WORD_SPLIT -- in the builds that hand lists on; the painting
  // builds file no lists and keep three lanes)
  if (p.cost_cnt != nullptr && l < ((!PAINT && p.split_bands) ? 4 : 3))
    filing_words_l = p.cost_cnt[l == 0 ? SWB_COST_WORD_KEY_LO(p.parity) : (l == 1 ? SWB_COST_WORD_KEY_SCALE(p.parity) : ((PAINT || l == 2) ? SWB_COST_WORD_COVER_SHIFT(ph) : SWB_COST_WORD_SPLIT(p.parity)))];
  if (p.ccost_list) cover_cost_housekeeping(p, block, ph_prev, ph, ph_next);
  // (the run lists' arena: every launch -- whether it lists runs or not -- leaves the NEXT launch's counter at zero)
  if (p.arena_head != nullptr && block == 0 && l == 0) p.arena_head[p.parity ^ 1] = 0u;
  if (p.cover_order) {
    const int sh = (int)(block & (SWB_COST_SHARDS - 1)), cap = (p.N + SWB_COST_SHARDS - 1) / SWB_COST_SHARDS;
    int bucket = 0;
    env = cost_ordered_entry(p.cost_cnt + cost_row1(ph_prev, sh),
                             as_const(p.ccost_list) + (size_t)(ph_prev * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS * cap, cap,
                             (int)(block >> 3), &bucket);
    if (env < 0) return;                                // (cannot happen: the host orders a launch only after one that filed all)
    prio_q = (p.prio_levels & 2) ? as_const(p.cost_cnt)[SWB_COST_WORD_COVER_PRIO(ph)] : 0u;
    if (prio_q) predicted = (uint32_t)(2 * bucket + 1) << (as_const(p.cost_cnt)[SWB_COST_WORD_COVER_SHIFT(ph_prev)] - 1u);
  }
  // at its end the wave files its environment under the cycles it took, for the order of the next cover launch
  auto file_cover_cost = [&]() __attribute__((always_inline)) {
    if (p.ccost_list) {
      const uint32_t cycles = (uint32_t)__builtin_amdgcn_s_memtime() - cycles0;
      const uint32_t width = (uint32_t)__builtin_amdgcn_readlane((int)filing_words_l, 2);     // (written by block 0 of the previous launch)
      if (l == 0) {
        const int key = (int)min(cycles >> width, (uint32_t)(SWB_COST_BUCKETS - 1));
        const int sh = env & (SWB_COST_SHARDS - 1);
        if ((cycles >> width) >= (uint32_t)SWB_COST_BUCKETS) atomicMax(&p.cost_cnt[SWB_COST_WORD_COVER_MAX(ph, sh)], cycles);
        const uint32_t pos = atomicAdd(&p.cost_cnt[cost_row1(ph, sh) + key], 1u);
        p.ccost_list[((size_t)(ph * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS + key) * ((p.N + SWB_COST_SHARDS - 1) / SWB_COST_SHARDS) + pos] = env;
      }
    }
  };
  auto reprioritise = [&]() __attribute__((always_inline)) {
    if (predicted) {
      const uint32_t elapsed = (uint32_t)__builtin_amdgcn_s_memtime() - cycles0;
      const int level = elapsed >= predicted ? 0 : (int)min((predicted - elapsed) >> prio_q, 3u);
      if (level != prio) {
        prio = level;
        if (level == 3) __builtin_amdgcn_s_setprio(3);
        else if (level == 2) __builtin_amdgcn_s_setprio(2);
        else if (level == 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
    }
  };
  reprioritise();
  unsigned char* wbase = smem;
  wave_lds<NW>* L = reinterpret_cast<wave_lds<NW>*>(wbase);
  edge_rec* edges = reinterpret_cast<edge_rec*>(wbase + ((sizeof(wave_lds<NW>) + (size_t)p.outrow_bytes + 15) & ~(size_t)15));
  uint32_t* spans = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(edges) +
                                                (((size_t)p.max_edges * sizeof(edge_rec) + 15) & ~(size_t)15));
  task_scratch* tscratch = reinterpret_cast<task_scratch*>(spans);
  int32_t* ovf = &L->ovf_slot;
  if (l == 0) *ovf = -1;
  const int S = p.S;

  // Centred paths of all sprites (float64 pairs): in the mask area while it is idle (P0/P1), or
  // in their own region when the masks are too small (tiny canvases).
  // (... else in the edge records' own storage: vertex k's centred path entry and edge k's record are both
  // 16 bytes at index k, and P1b's first sweep reads entry k before it writes record k from the same lane)
  double2* cpath = p.cpath_in_masks ? reinterpret_cast<double2*>(L->T) : reinterpret_cast<double2*>(edges);
  static_assert(sizeof(double2) == sizeof(edge_rec), "centred paths alias the edge records");

  // ------------------------------------------------------------------ P0: state
  // (with the state's two rounds of loads, the kernel's own: the shape table P1b looks up whole, lane i = entry i; the fill colours)
  uint32_t err = 0;
  const double shdmin_tab_l = (l < SWB_MAX_SHAPES) ? p.shape_dmin[l] : 0.0;
  // (... and what keeping the lists takes, swb_params::list_epoch: lane g < SWB_MAX_CG the cost the list of column group g was
  // filed under, lane SWB_MAX_CG the header's stamp, the lane behind it the cycles of the wave that built the lists, the next
  // one the state of the frame cache (SWB_RHDR_FRAME).  It depends on nothing but `env`; a plain load, not as_const: this wave
  // writes the words again at its end.)
  // The words wait in LDS (wave_lds::outrow is idle until P1b), not in a register across the state phase.
  if constexpr (!PAINT) {
    if (p.list_epoch != 0u && l <= SWB_MAX_CG + 2) L->outrow[l] = p.rhdr[(size_t)env * SWB_RHDR_DWORDS + SWB_RHDR_COST + l];
  }
  const uint32_t task_rec_l = load_task_record(p, env);
  env_state es = load_env_state<OV>(p, env, tscratch);
  park_task_record(p, task_rec_l, tscratch);
  const int n = es.n, nv_l = es.nv_l;
  const double scale_l = es.scale_l;
  uint32_t rgb_reg = 0u;                                // lane s: fill colour of sprite s
  if (l < S) rgb_reg = p.p_rgb[(size_t)es.en * S + l];
  if (l >= n) rgb_reg = 0u;

  // ------------------------------------------------------------------ P1a: centred paths
  // all vertices of all sprites, 64 per pass (cross-lane reads with every lane active)
  const double dmin_any = __shfl(shdmin_tab_l, es.sh_idx, 64);
  double dmin_l = (l < n) ? dmin_any : 0.0;              // P1b: can two vertices share a pixel?
  if constexpr (OV) { if (es.ov) dmin_l = 0.0; }        // an overridden path is arbitrary: always the general corner scan
  int voff_l = nv_l;                                    // inclusive prefix sum over lanes (sprites)
  for (int o = 1; o < SWB_TUNED_SPRITES; o <<= 1) { const int t = __shfl_up(voff_l, o, 64); if (l >= o) voff_l += t; }
  const int vtotal = __builtin_amdgcn_readlane(voff_l, SWB_TUNED_SPRITES - 1);
  voff_l -= nv_l;                                       // exclusive
  for (int base = 0; base < vtotal; base += 64) {
    const int k = base + l;
    int sid = 0;
    for (int s2 = 1; s2 < n; ++s2) if (k >= __builtin_amdgcn_readlane(voff_l, s2)) sid = s2;
    // cross-lane reads with every lane active (a disabled source lane would read as 0)
    const int i = k - __shfl(voff_l, sid, 64);
    const int so = __shfl(es.so_l, sid, 64);
    const double sc = __shfl(scale_l, sid, 64), ca = __shfl(es.ca_l, sid, 64), sa = __shfl(es.sa_l, sid, 64);
    if (k < vtotal) {
      double cx, cy;
      bool from_table = true;
      if constexpr (OV) {
        if (es.ov) {                                    // the path the setters left (host arithmetic, swb.hip)
          const double* q = p.ov_cpath + (((size_t)env * S + sid) * SWB_MAX_SHAPE_VERTS + i) * 2;
          cx = q[0]; cy = q[1];
          from_table = false;
        }
      }
      if (from_table) centered_vertex(p, so, i, sc, ca, sa, cx, cy);
      cpath[k] = make_double2(cx, cy);
    }
  }
  wave_sync();
  SWB_HOOK_PHASE_END(3)

  // sprite.py:113-115 contains_point of sprite s2 (wave-uniform): its centred path is in the table P1a built
  auto hit = [&](int s2, double tx, double ty) __attribute__((always_inline)) {
    return contains_point_wave(cpath + __builtin_amdgcn_readlane(voff_l, s2), __builtin_amdgcn_readlane(nv_l, s2), tx, ty);
  };
  const step_cost sc = act_and_move(p, env, es, hit);
  const double px = es.px, py = es.py;
  SWB_HOOK_PHASE_END(4)
  if (p.render_only != 1 && es.active) {                // (no part in the step: no task, no outputs -- skipped, not masked)
    err |= finish_step<OV, true, SETS>(p, env, es, sc, tscratch);
    wave_sync();                                        // (the scratch aliases the span lists)
  }
  SWB_HOOK_PHASE_END(5)
  if (p.obs == nullptr) {
    if (l == 0 && p.error && err) p.error[env] |= (uint8_t)err;        // sticky: the caller clears
    return;
  }

  // The end of a wave that hands lists to the second kernel, whether it built them or kept them.
  // Filing, twice: lane g files the task (environment, column group g) for the resample kernel under the length of ITS list (the
  // groups of a wide image see different sprites), lane 0 the environment for the next cover launch under the cycles this wave
  // took.  Both are a returning atomic followed by a store at the position it returned: the two atomics are issued back to back
  // so that their round trips overlap.
  // Small batches (nbands > 1, swb_params::band_tasks): the second kernel's task is one BAND of a list, filed by lane g * nbands + b
  // under the cost of the band's own part -- the units between its first run and the next band's, plus its share of the canvas
  // rows it walks beyond that (5 / 16 of the next band: 25 of 80 rows; none at anti_aliasing = 1), 4 per unit = 2 per byte of list
  // like the whole-list cost.  (Filed per list, the four bands of an environment ended up on one SIMD -- workgroups x, x + 256, ...
  // of a 1024-environment launch share a compute unit -- and a SIMD's work was one environment's whole list: 56 k .. 267 k cycles
  // over the SIMDs, the launch as long as its heaviest scene; gpurun_out/r06n/timeline_1024.json.)  The band starts come from
  // their copy in LDS (`bst`; reading the header back takes an agent-scope fence, which writes the XCD's L2 back: measured, the
  // cover kernel of 4096 environments 0.052 -> 0.133 ms).
  // cost_l: lane g, the cost of the list of column group g; built_cycles: 0, or (kept lists) the cycles of the wave that built
  // them, in place of this wave's own; copied: the environment's frame is the copy this launch's copy workgroups make
  // (swb_params::spec_copy, SWB_RHDR_FRAME = 2) -- the wave files NO task for the second kernel, only its environment for the
  // next cover launch.  Then the overflow slot goes back and the error flags out.
  [[maybe_unused]] auto file_lists = [&](int cost_l, const uint32_t* bst, uint32_t built_cycles, bool copied) __attribute__((always_inline)) {
    // Split bands (swb_params::split_bands): the band tasks only where the launch's word says split; else one WHOLE task per
    // column group, under the whole list's cost.  Lane 0 counts the wave's frames for the next launch's word.
    const bool whole = p.split_bands && (copied || __builtin_amdgcn_readlane((int)filing_words_l, 3) == 0);
    const bool bt = bst != nullptr && !whole;
    const int ntask = bt ? p.ncg * p.nbands : p.ncg;
    const bool file0 = p.cost_cnt != nullptr && l < ntask && !copied, file1 = p.ccost_list != nullptr && l == 0;
    const int sh = env & (SWB_COST_SHARDS - 1);
    int task_cost = cost_l, task_bits = l << 24;
    if (bt) {
      wave_sync();
      const int g2 = min(l / p.nbands, p.ncg - 1), b2 = l - (l / p.nbands) * p.nbands;
      const uint32_t* bg = bst + g2 * SWB_BST_STRIDE;
      const int u0 = (int)bg[b2], u1 = (int)bg[min(b2 + 1, p.nbands)], u2 = (int)bg[min(b2 + 2, p.nbands)];
      task_cost = 4 * max((u1 - u0) + (p.AA == 1 ? 0 : (((u2 - u1) * 5) >> 4)), 0);
      task_bits = (g2 << 24) | (b2 << 26);
    }
    if (whole) task_bits |= SWB_TASK_WHOLE;
    const int key0 = cost_key(task_cost, (uint32_t)__builtin_amdgcn_readlane((int)filing_words_l, 0), (uint32_t)__builtin_amdgcn_readlane((int)filing_words_l, 1));
    int key1 = 0;
    uint32_t cycles = built_cycles;
    if (p.ccost_list) {
      if (built_cycles == 0u) cycles = (uint32_t)__builtin_amdgcn_s_memtime() - cycles0;
      const uint32_t width = (uint32_t)__builtin_amdgcn_readlane((int)filing_words_l, 2);      // (written by block 0 of the previous launch)
      key1 = (int)min(cycles >> width, (uint32_t)(SWB_COST_BUCKETS - 1));
      if (l == 0 && (cycles >> width) >= (uint32_t)SWB_COST_BUCKETS) atomicMax(&p.cost_cnt[SWB_COST_WORD_COVER_MAX(ph, sh)], cycles);
    }
    uint32_t pos0 = 0u, pos1 = 0u;
    if (file0) pos0 = atomicAdd(&p.cost_cnt[cost_row0(p.parity, sh) + key0], 1u);
    if (file1) pos1 = atomicAdd(&p.cost_cnt[cost_row1(ph, sh) + key1], 1u);
    if (p.split_bands && !copied && p.cost_cnt != nullptr && l == 0) atomicAdd(&p.cost_cnt[SWB_COST_WORD_SPLIT_CNT(p.parity, sh, (env >> 3) & (SWB_COST_BUCKETS - 1))], (uint32_t)p.ncg);
    // (SWB_LIST_STATS: the counters keep the meaning they had while tasks of the second kernel made the copies -- what those would
    // have counted: a task per column group, and per band where the grid or the filing is per band; split bands: whole copies)
    if (copied && p.frame_stats && l == 0) {
      atomicAdd(&p.frame_stats[0], (unsigned long long)(p.split_bands ? p.ncg : p.ncg * p.nbands));
      if (p.split_stats) atomicAdd(&p.split_stats[2], (unsigned long long)p.ncg);
    }
    if (file0) p.cost_list[((size_t)(p.parity * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS + key0) * p.cost_cap + pos0] = env | task_bits;
    if (file1) p.ccost_list[((size_t)(ph * SWB_COST_SHARDS + sh) * SWB_COST_BUCKETS + key1) * ((p.N + SWB_COST_SHARDS - 1) / SWB_COST_SHARDS) + pos1] = env;
    if (l == 0) ovf_slot_release(p, ovf);
    if (p.error) {
      uint32_t e = err & ~SWB_INT_NEED_SLOT;
      for (int o = 32; o > 0; o >>= 1) e |= (uint32_t)__shfl_xor((int)e, o, 64);
      if (l == 0 && e) p.error[env] |= (uint8_t)e;                       // sticky: the caller clears
    }
    return cycles;
  };

  // ------------------------------------------------------------------ kept lists (swb_params::list_epoch)
  // The lists this environment's header describes were built under the current epoch, without an error and inside their own
  // parts (the stamp says so), this launch did not reset the environment -- pool entry and sprite count are then the ones they
  // were built from -- and no sprite's position differs BITWISE from the one loaded (step_cost::changed: a missed click, a zero
  // motion, a move clipped back onto the same value, zero velocities are all the same to the test).  Then P1b, P2 and emit_runs would write the bytes that
  // are in memory already: the wave files the lists as they are.  The header's words were written by an earlier launch (no
  // fence), and the arena is not touched.  The second kernel runs for this environment as for every other.
  if constexpr (!PAINT) {
    bool keep = false;
    uint32_t keep_words_l = 0u;
    if (p.list_epoch != 0u) {
      if (l <= SWB_MAX_CG + 2) keep_words_l = L->outrow[l];
      keep = (uint32_t)__builtin_amdgcn_readlane((int)keep_words_l, SWB_MAX_CG) == p.list_epoch && __ballot(es.first) == 0ull && !sc.changed;
    }
    if (p.list_stats != nullptr && l == 0) atomicAdd(&p.list_stats[keep ? 0 : 1], 1ull);
    if (keep) {
      // the frame (SWB_RHDR_FRAME): kept once, the resample waves of this launch fill the cache; kept again, the frame is the copy
      // this launch's copy workgroups make of it (spec_copy_group: they copied on the old word, 1 or 2) and no task is filed
      // (written only where it changes: a wave that keeps on through a still period writes nothing at all, as before)
      const uint32_t frame_word_was = (uint32_t)__builtin_amdgcn_readlane((int)keep_words_l, SWB_MAX_CG + 2);
      const uint32_t frame_word = p.frame_cache ? min(frame_word_was + 1u, 2u) : 0u;
      uint32_t* bst = nullptr;
      // the band starts (and, in slot nbands, the list's end) from the header -- split bands: not for a wave that files whole
      // tasks (file_lists decides the same way), which is nearly every wave that keeps (a round trip to memory at the wave's end, with nothing behind it to hide it)
      // -- and not for a wave whose frame is the copy: it files no task at all
      const bool copied = frame_word == 2u && p.spec_copy != 0;
      const bool files_whole = p.split_bands && (frame_word == 2u || __builtin_amdgcn_readlane((int)filing_words_l, 3) == 0);
      if (p.band_tasks && !files_whole && !copied) {
        bst = L->outrow + 64;
        const uint32_t* hg = p.rhdr + (size_t)env * SWB_RHDR_DWORDS + SWB_RHDR_GROUPS;
        const int g = l / SWB_BST_STRIDE, b = l - g * SWB_BST_STRIDE;
        if (g < p.ncg && b <= p.nbands) bst[l] = hg[g * SWB_RHDR_GSTRIDE + (b < p.nbands ? 1 + b : 0)];
      }
      if (l == 0 && frame_word != frame_word_was) p.rhdr[(size_t)env * SWB_RHDR_DWORDS + SWB_RHDR_FRAME] = frame_word;
      file_lists((int)keep_words_l, bst, max((uint32_t)__builtin_amdgcn_readlane((int)keep_words_l, SWB_MAX_CG + 1), 1u), copied);
      return;
    }
  }

  // ------------------------------------------------------------------ P1b: canvas edges
  build_all_edges<NW>(p, L, edges, cpath, spans, n, vtotal, voff_l, nv_l, px, py, dmin_l, scale_l, rgb_reg, err);
  // the mask arrays start (and are kept) zero; they may have held the centred paths until here
#pragma unroll
  for (int w = 0; w < SWB_NWA(NW); ++w) { L->T[w][l] = 0u; L->Px[w][l] = 0u; }
  wave_sync();

  // Scenes of many sprites are the ones whose rows outgrow the span lists: they take their overflow slot up
  // front (one atomic) instead of paying a second scan of the first batch that needs it.
  if (n >= SWB_EAGER_OVF_SPRITES && l == 0) *ovf = ovf_slot_alloc(p);
  // lane s < n: sprite s's scan range and packed raster parameters for P2 (see coverage_batch2)
  int sp_ymin = 0x7fffffff, sp_ymax = -0x7fffffff, sp_e0 = 0;
  uint32_t sp_a = 0u;
  if (l < n) {
    const sprite_rec r = L->spr[l];
    // lanes per edge of the edge-lane scatter: G = 64 / n_edges (1 .. 32), so that lane l serves edge l / G -- computed there as
    // (l * ceil(2^16 / G)) >> 16, which is exact for l < 64: the rounding adds less than 64 / 2^16 to l / G, and l / G is at
    // least 1 / G >= 1 / 32 below the next integer.  The reciprocal is 2^16 itself for G = 1 (shapes of 33 .. 64 edges): 17 bits,
    // above the 12 bits of the edge slot (at most SWB_TUNED_SPRITES * SWB_MAX_SHAPE_VERTS = 1024 slots).
    static_assert(SWB_TUNED_SPRITES * SWB_MAX_SHAPE_VERTS <= 4096 && SWB_MAX_SHAPE_VERTS <= 64, "packing of sp_e0 / lanes per edge");
    const int lanes_per_edge = max(64 / max(r.n_edges, 2), 1);
    sp_ymin = r.ymin; sp_ymax = r.ymax;
    sp_e0 = r.edge_off | (((65536 + lanes_per_edge - 1) / lanes_per_edge) << 12);
    sp_a = (uint32_t)r.w0 | ((uint32_t)r.w1 << 5) | ((uint32_t)r.n_edges << 10) | ((uint32_t)min(r.max_edge_rows, 127) << 17) |
           ((uint32_t)lanes_per_edge << 24);
  }
  // the hand-off header: per sprite the colour's difference to the background as three signed 10-bit fields
  // (horizontal pass of the resample kernel) and the colour itself (fill kernel)
  uint32_t* hdr = p.rhdr + (size_t)env * SWB_RHDR_DWORDS;
  if (l < SWB_TUNED_SPRITES && !PAINT) {
    hdr[l] = (uint32_t)(((int)(rgb_reg & 255) - (int)(p.bg & 255)) & 0x3ff) |
             ((uint32_t)(((int)((rgb_reg >> 8) & 255) - (int)((p.bg >> 8) & 255)) & 0x3ff) << 10) |
             ((uint32_t)(((int)((rgb_reg >> 16) & 255) - (int)((p.bg >> 16) & 255)) & 0x3ff) << 20);
    hdr[SWB_TUNED_SPRITES + l] = rgb_reg;
  }
  SWB_HOOK_PHASE_END(1)
  reprioritise();

  // ------------------------------------------------------------------ P2: coverage, batch by batch -> run lists
  // Batches of 64 canvas rows.  Where rows without spans are not listed (black background, or anti_aliasing = 1) a
  // batch starts at the next row some sprite covers: the first sprite below the previous batch is never split over
  // two batches and empty stretches cost nothing.
  if constexpr (PAINT) {
    // anti_aliasing = 1 and an image of up to 64 columns: the canvas IS the image (pil_renderer.py:84 resizes to the same
    // size, i.e. copies), a row is 48 dwords -- the wave paints it itself, batch by batch, instead of listing runs for a
    // second kernel (one launch less, no lists through HBM).  Lanes = columns; a row is packed in registers (4 lanes =
    // 12 bytes = 3 dwords: one quad-permute DPP move + one v_perm_b32) and stored flipped (np.flipud :90); rows no sprite
    // covers are background; every pixel is written exactly once.
    const int nd1 = (p.Wo * 3) >> 2;                                      // dwords per row (Wo % 4 == 0)
    unsigned char* const frame1 = p.obs + (size_t)env * p.Wo * p.Ho * 3;      // (rows are stored through a 32-bit BYTE offset from this
                                                                               // uniform base: no 64-bit address arithmetic per row)
    const uint32_t row_bytes1 = 4u * (uint32_t)nd1;
    const uint32_t pack_sel1 = ((l & 3) == 0) ? 0x04020100u : (((l & 3) == 1) ? 0x05040201u : 0x06050402u);
    const bool pack_store1 = ((l & 3) != 3) && (l < p.Wo);
    uint32_t off1 = 4u * (uint32_t)((p.Ho - 1) * nd1 + 3 * (l >> 2) + (l & 3));    // canvas row 0 is image row Ho - 1
    auto pack1 = [&](uint32_t col) __attribute__((always_inline)) {
      const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)col, 0xF9, 0xf, 0xf, false);   // quad_perm:[1,2,3,3]
      return __builtin_amdgcn_perm(nb, col, pack_sel1);
    };
    const uint32_t bg_dw1 = pack1(p.bg);
    int y_next = 0;                                                       // first row not written yet
    for (int yb = 0;; yb += 64) {
      int v = (l < n && sp_ymax >= yb) ? max(sp_ymin, yb) : 0x7fffffff;  // the next row some sprite covers
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x111, 0xf, 0xf, false));   // row_shr:1
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x112, 0xf, 0xf, false));   // row_shr:2
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x114, 0xf, 0xf, false));   // row_shr:4
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x118, 0xf, 0xf, false));   // row_shr:8
      yb = min(__builtin_amdgcn_readlane(v, SWB_TUNED_SPRITES - 1), p.Hc);
      for (; y_next < yb; ++y_next) { if (pack_store1) *reinterpret_cast<uint32_t*>(frame1 + off1) = bg_dw1; off1 -= row_bytes1; }    // rows above the batch
      if (yb >= p.Hc) break;
      row_spans rs;
      coverage_batch2<NW>(p, L, edges, spans, ovf, n, yb, sp_ymin, sp_ymax, sp_a, sp_e0, rs, err);
      SWB_RESCAN_WITH_OVERFLOW_SLOT()
      const int rows = min(64, p.Hc - yb);
      const unsigned long long covered_rows = __ballot(rs.cnt != 0u);
      for (int r = 0; r < rows; ++r) {
        uint32_t dw = bg_dw1;
        if ((covered_rows >> r) & 1ull) {
          const int ns = __builtin_amdgcn_readlane((int)rs.cnt, r);      // (>= 1: the row's bit is set)
          uint32_t col = p.bg;
          // (a row's visible spans are disjoint: any order.  The three in registers are taken straight-line, as in the second
          // kernels -- the loop over get_span's switch cost the row four taken scalar branches per span)
          auto paint1 = [&](uint32_t sp) __attribute__((always_inline)) {
            const int a = sp & 1023, b = (sp >> 10) & 1023;
            const uint32_t rgb = (uint32_t)__builtin_amdgcn_readlane((int)rgb_reg, (int)(sp >> 20));
            if (l >= a && l < b) col = rgb;
          };
          paint1((uint32_t)__builtin_amdgcn_readlane((int)rs.s0, r));
          if (ns >= 2) {
            paint1((uint32_t)__builtin_amdgcn_readlane((int)rs.s1, r));
            if (ns >= 3) {
              paint1((uint32_t)__builtin_amdgcn_readlane((int)rs.s2, r));
              for (int m = SWB_REG_SPANS; m < ns; ++m) paint1(get_span(p, spans, ovf, rs, m, r));
            }
          }
          dw = pack1(col);
        }
        if (pack_store1) *reinterpret_cast<uint32_t*>(frame1 + off1) = dw;
        off1 -= row_bytes1;
      }
      y_next = yb + rows;
      reprioritise();
    }
    file_cover_cost();
    if (l == 0) ovf_slot_release(p, ovf);
    if (p.error) {
      uint32_t flags = err & ~SWB_INT_NEED_SLOT;
      for (int o = 32; o > 0; o >>= 1) flags |= (uint32_t)__shfl_xor((int)flags, o, 64);
      if (l == 0 && flags) p.error[env] |= (uint8_t)flags;               // sticky: the caller clears
    }
    return;
  } else {
  uint32_t* runs_env = p.runs + (size_t)env * p.ncg * p.run_cap * 2;
  // lane g, for the list of column group g: the unit it stands at (counted from the first unit of the list's own part; beyond
  // run_cap: the list has moved to the arena), its next band (+ where it lives, see emit_runs), its cost
  int base_l = 0, band_l = 0, cost_l = 0;
  static_assert(64 + SWB_MAX_CG * SWB_BST_STRIDE <= 132, "the band starts borrow wave_lds::outrow behind the scatter's 64 slots");
  uint32_t* const bst = p.band_tasks ? L->outrow + 64 : nullptr;
  const bool skip_empty = (p.bg == 0u) || p.AA == 1;
  for (int yb = 0;; yb += 64) {
    if (skip_empty) {
      int v = (l < n && sp_ymax >= yb) ? max(sp_ymin, yb) : 0x7fffffff;
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x111, 0xf, 0xf, false));   // row_shr:1
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x112, 0xf, 0xf, false));   // row_shr:2
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x114, 0xf, 0xf, false));   // row_shr:4
      v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x118, 0xf, 0xf, false));   // row_shr:8
      yb = __builtin_amdgcn_readlane(v, SWB_TUNED_SPRITES - 1);
    }
    if (yb >= p.Hc) break;
    row_spans rs;
    coverage_batch2<NW>(p, L, edges, spans, ovf, n, yb, sp_ymin, sp_ymax, sp_a, sp_e0, rs, err);
    SWB_RESCAN_WITH_OVERFLOW_SLOT()
    emit_runs(p, spans, ovf, rs, yb, env, runs_env, hdr, bst, base_l, band_l, cost_l, err);
    reprioritise();
  }
  // list lengths; bands that start below the last batch begin at the end of the list
  if (l < p.ncg) {                                     // lane g finishes the list of column group g
    hdr[SWB_RHDR_GROUPS + l * SWB_RHDR_GSTRIDE] = (uint32_t)base_l;
    for (int b = band_l & 15; b < p.nbands; ++b) hdr[SWB_RHDR_GROUPS + l * SWB_RHDR_GSTRIDE + 1 + b] = (uint32_t)base_l;
    if (bst) for (int b = band_l & 15; b <= p.nbands; ++b) bst[l * SWB_BST_STRIDE + b] = (uint32_t)base_l;      // (slot nbands: the list's end)
    // the sentinel: a run on row 0xffff, below every canvas row (the lists have one unit of room for it)
    *reinterpret_cast<uint2*>(runs_env + (size_t)l * p.run_cap * 2 + 2 * (long long)base_l) = make_uint2(0xffffu, 0u);
  }
  // the stamp, behind the sentinels: a later launch may keep these lists if they were built without an error, every one of them
  // inside its own part (a list in the arena is overwritten two launches later), and under an epoch (swb_params::list_epoch)
  {
    const bool flawed_l = (err & ~SWB_INT_NEED_SLOT) != 0u || (l < p.ncg && ((uint32_t)band_l >> 4) != 0u);
    const bool stamped = p.list_epoch != 0u && __ballot(flawed_l) == 0ull;
    if (l <= SWB_MAX_CG) hdr[SWB_RHDR_COST + l] = l < SWB_MAX_CG ? (uint32_t)cost_l : (stamped ? p.list_epoch : 0u);
    if (l == SWB_MAX_CG + 2) hdr[SWB_RHDR_FRAME] = 0u;       // (new lists: the cache does not hold their frame)
  }
  const uint32_t own_cycles = file_lists(cost_l, bst, 0u, false);
  if (l == 0 && p.list_epoch != 0u) hdr[SWB_RHDR_CYCLES] = own_cycles;
  }   // !PAINT
}
#ifndef SWB_SETS_PASS      // ---- (the rest of the file, down to the many-sprite state kernel, is not part of the pass)
// the build of handles with task sets; defined by the pass, explicitly instantiated in swb_wide.hip at every width
template <int NW, bool PAINT = false>
__global__ void swb_cover_sets_kernel(const swb_params p);

// --------------------------------------------------------------------------------------------
// Kernel 2 of a step, "resample" (anti_aliasing > 1): P3 + P4 for one (environment, group of 64 output columns,
// band of output rows) per wave -- Pillow's two-pass LANCZOS reduction (Resample.c, horizontal pass first, uint8
// in between) evaluated from the run lists, never from a canvas:
//   horizontal  lanes = output columns; a run's row is sum over its spans of (colour - background) * (P[end] -
//               P[start]) with P the column's prefix-summed 22-bit coefficients (one v_med3 + one LDS read per
//               index), plus the background total; clip -> uint8;
//   vertical    the uint8 result times the run's coefficient sums (difference of two rows of the prefix table
//               v_pfx: two scalar loads whatever the run length) into the VS output rows in flight, kept as
//               3 x VS accumulators per lane in registers; slot = output row % VS, so rows never move;
//   store       a finished row is packed in registers (4 lanes = 12 bytes = 3 dwords: one quad-permute DPP move
//               + one v_perm_b32) and written flipped (np.flipud, pil_renderer.py:90), coalesced.
// The wave needs nothing but the run list, 16 colours and the tables: 8 waves per SIMD.  A band starts with the
// output rows already in flight at its first canvas row; those above the band are completed without a store.
// --------------------------------------------------------------------------------------------
// The loop is written for the SCALAR unit as much as for the vector ALU (a SIMD issues about one instruction of
// each kind per 4 cycles; the first version of this kernel retired 92 scalar instructions per run against 45
// vector ones and was bound by them): lists end with a sentinel run instead of a length test, the list position
// and the table rows are 32-bit byte offsets of scalar loads, the accumulator slot of the row being finished is
// a compile-time constant (the row loop is unrolled VS times; bands start on a multiple of VS rows in flight),
// a slot that received nothing since its restart is recognised by the list position not having moved.
// A run record is { row | rows-1 << 16 | continuation << 23 | spans << 24, span 0 } [{ span 1, span 2 } ...] (swb_params::runs).  A
// continuation run -- the rows below a forced run end that have the spans of the run before it -- is one unit: the loop skips
// from the two table loads straight to the vertical pass with the h[0..2] it holds (clipped, live across iterations); the
// list position moves by one unit, so the "untouched slot" test above works as before.
typedef uint32_t swb_u4 __attribute__((ext_vector_type(4), aligned(8)));      // a run record starts on an 8-byte unit
typedef int32_t swb_i8 __attribute__((ext_vector_type(8), aligned(32)));
template <int VS>
__global__ void __launch_bounds__(SWB_WAVE* SWB_RS_WAVES_PER_BLOCK, SWB_RS_WAVES_PER_SIMD)
swb_resample_kernel(const swb_params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = rfl(threadIdx.x >> 6);                        // (wave-uniform: everything below is scalar control flow)
  const int l = lane_id();
  const int task = blockIdx.x * SWB_RS_WAVES_PER_BLOCK + wave;
  int band = blockIdx.y;
  // consecutive blocks of a shard take tasks (environment, column group[, band: swb_params::band_tasks]) of decreasing cost: the
  // eight waves of a SIMD get one of every octile.  (Without cost ordering: blockIdx.z is the column group.)
  int env = task < p.N ? task : -1, g = blockIdx.z;
  bool whole = false;                                            // (split bands: the task is the frame's whole rows, SWB_TASK_WHOLE)
  if (p.cost_cnt) {
    const int first = dealt_block(p, (int)(blockIdx.x >> 3), (int)(gridDim.x >> 3)) * SWB_RS_WAVES_PER_BLOCK;
    int filed = 0;
    // (the filed count and the whole bit are taken on every handle: one readlane and one bit test.  OPEN QUESTION: taking them only
    // in the mode was built and measured once -- `cluster_s5:65536:5`, where the mode is off, had its resample kernel 4.5 % longer in
    // four of six rounds, against +0.06 % for this form (profiles/r20_split_bands.md section 6).  The cause is not known: the rounds
    // were bimodal, so it may be where the code lands rather than the six instructions.  Not a settled trade-off; measure again.)
    env = cost_ordered_env(p, p.parity, (int)(blockIdx.x & (SWB_COST_SHARDS - 1)), first + wave, &filed);
    if (env >= 0) {
      whole = (env & SWB_TASK_WHOLE) != 0;
      if (p.band_tasks) band = rfl((env >> 26) & 7);
      g = (env >> 24) & 3; env &= 0xffffff;
    }
    if (blockIdx.y == 0) cost_housekeeping(p, (int)blockIdx.x, wave);
    // Split bands: the grid covers the worst case, every environment in bands -- most workgroups of a launch have no task at all.
    // Tasks are dealt in index order, so a workgroup whose first wave has none is empty: it leaves before the table and the barrier.
    if (p.split_bands && first >= filed) return;
  }
  int32_t* pfx = reinterpret_cast<int32_t*>(smem);               // block-shared prefix table of the horizontal pass
  for (int i = threadIdx.x; i < p.h_pfx_len; i += blockDim.x) pfx[i] = p.h_pfx[i];
  __syncthreads();
  if (env < 0) return;
  const int o_lo = as_const(p.band_lo)[band], o_hi = as_const(p.band_lo)[whole ? p.nbands : band + 1];
  if (o_lo >= o_hi) return;
  cptr<uint32_t> hdr = as_const(p.rhdr) + (size_t)env * SWB_RHDR_DWORDS;
  // The frame cache (swb_params::frame_cache), decided once and wave-uniform from the word the cover wave left (SWB_RHDR_FRAME):
  // 0 resample, as ever; 1 resample, then leave the wave's rectangle -- output rows [o_lo, o_hi) of column group g -- in the
  // cache; 2 copy the rectangle from the cache to the frame and return: no list, no prefix table, no lane constants.  (2 is met only
  // on handles that dispatch without cost order, whose grid has a wave for every environment: where tasks are filed, the cover
  // launch made the copy and the environment filed none -- swb_params::spec_copy.)
  const uint32_t frame_mode = p.frame_cache ? hdr[SWB_RHDR_FRAME] : 0u;
  const uint32_t rect_row_bytes = 3u * (uint32_t)p.Wo, rect_seg_bytes = 3u * (uint32_t)min(64, p.Wo - 64 * g);
  const size_t frame_off = (size_t)env * p.Wo * p.Ho * 3 + (size_t)(p.Ho - o_hi) * rect_row_bytes + 192u * (uint32_t)g;
  const uint32_t cycles0 = p.frame_stats ? (uint32_t)__builtin_amdgcn_s_memtime() : 0u;
  // (the counts are of FRAMES where an environment's tasks differ in number -- split bands: the whole task or band 0 counts)
  if (p.frame_stats && l == 0 && (!p.split_bands || whole || band == 0)) atomicAdd(&p.frame_stats[frame_mode == 2u ? 0 : (frame_mode == 1u ? 1 : 2)], 1ull);
  if (p.split_stats && l == 0) atomicAdd(&p.split_stats[!whole ? 1 : (frame_mode == 2u ? 2 : 0)], 1ull);
  if (frame_mode == 2u) {
    copy_frame_rect(p.frame_cache + frame_off, p.obs + frame_off, rect_row_bytes, rect_seg_bytes, o_hi - o_lo, p.obs_aligned16 != 0);
    if (p.frame_stats && l == 0) atomicAdd(&p.frame_stats[3], (unsigned long long)((uint32_t)__builtin_amdgcn_s_memtime() - cycles0));
    return;
  }
  const uint32_t dpk_reg = (l < SWB_TUNED_SPRITES) ? p.rhdr[(size_t)env * SWB_RHDR_DWORDS + l] : 0u;   // lane s: sprite s
  uint32_t uo = 8u * hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE + 1 + band];                           // byte offset of the next run
  // Wave priority by the list left to walk.  A SIMD issues from its oldest wave first, so the waves of a launch finish one after
  // the other and the last one alone, far below the SIMD's rate; with the priority (0..3) following the remaining work --
  // "longest remaining time first" -- they finish together instead.  One level = 2^prio_shift bytes of list (about half a
  // mean list; from the previous launch's histogram, cost_housekeeping), re-evaluated at every finished output row.
  const uint32_t u_end = 8u * hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE + ((!whole && band + 1 < p.nbands) ? 2 + band : 0)];
  const uint32_t prio_shift = p.cost_cnt ? as_const(p.cost_cnt)[SWB_COST_WORD_PRIO_SHIFT(p.parity)] : 0u;
  int prio = prio_shift ? (int)min((u_end - uo) >> prio_shift, 3u) : 0;
  if (p.frame_stats && l == 0) atomicAdd(&p.frame_stats[5], (unsigned long long)(u_end - uo));
  if (prio == 3) __builtin_amdgcn_s_setprio(3);
  else if (prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (prio == 1) __builtin_amdgcn_s_setprio(1);
  cptr<unsigned char> runs = reinterpret_cast<cptr<unsigned char>>(as_const(p.runs) + ((size_t)env * p.ncg + g) * p.run_cap * 2);
  cptr<unsigned char> vpfx = reinterpret_cast<cptr<unsigned char>>(as_const(p.v_pfx));
  const int bg0 = p.bg & 255, bg1 = (p.bg >> 8) & 255, bg2 = (p.bg >> 16) & 255;
  // per-lane constants of the horizontal pass: P_o(x) = pfx[htbl + clamp(x - hxmin, 0, hcnt)] = pbase[clamp(x, hlo, hhi)]
  const int o = min(64 * g + l, p.Wo - 1);
  const int hxmin = p.h_xmin[o], hcnt = p.h_cnt[o], htbl = p.h_tbl[o];
  const int hlo = hxmin, hhi = hxmin + hcnt;
  const int32_t* pbase = pfx + (htbl - hxmin);
  const int tot = pfx[htbl + hcnt];
  const int bgtot0 = bg0 * tot + SWB_HALF, bgtot1 = bg1 * tot + SWB_HALF, bgtot2 = bg2 * tot + SWB_HALF;
  int acc[3][VS];
  uint32_t mark[VS];                                   // list position at the slot's restart
#pragma unroll
  for (int k = 0; k < VS; ++k) { acc[0][k] = SWB_HALF; acc[1][k] = SWB_HALF; acc[2][k] = SWB_HALF; mark[k] = uo; }
  int r_first = as_const(p.band_first)[band];          // oldest in-flight output row: a multiple of VS rows before ... slot 0
  int next_end = as_const(p.v_end)[r_first], next_end2 = as_const(p.v_end)[r_first + 1];   // (the table is padded)
  const bool black = (p.bg == 0u);
  // this lane's dword of the output row being finished; rows are written bottom-up (np.flipud :90)
  const int nd = (p.Wo * 3) >> 2;                      // Wo*3 is a multiple of 4 (Wo % 4 == 0)
  unsigned char* const frame_bytes = p.obs + (size_t)env * p.Wo * p.Ho * 3;
  const uint32_t pack_sel = ((l & 3) == 0) ? 0x04020100u : (((l & 3) == 1) ? 0x05040201u : 0x06050402u);
  const bool pack_store = ((l & 3) != 3) && (64 * g + l < p.Wo);
  const uint32_t row_bytes = 4u * (uint32_t)nd;
  uint32_t dst_off = 4u * (uint32_t)((p.Ho - 1 - o_lo) * nd + 48 * g + 3 * (l >> 2) + (l & 3));      // in bytes
  // horizontal-pass contribution of one visible span to this lane's output column
  auto add_span = [&](uint32_t sp, int (&h)[3]) __attribute__((always_inline)) {
    const int a = sp & 1023, b = (sp >> 10) & 1023;
    const int dpk = __builtin_amdgcn_readlane((int)dpk_reg, (int)(sp >> 20));
    // (the three signed 10-bit fields: shifted up as unsigned -- a signed shift into the sign bit is undefined before C++20 --,
    // then down arithmetically: the same two instructions per field)
    const uint32_t dpu = (uint32_t)dpk;
    const int d0 = (int)(dpu << 22) >> 22, d1 = (int)(dpu << 12) >> 22, d2 = (int)(dpu << 2) >> 22;
    const int w = pbase[med3_su(b, hlo, hhi)] - pbase[med3_su(a, hlo, hhi)];
    h[0] += __mul24(d0, w); h[1] += __mul24(d1, w); h[2] += __mul24(d2, w);   // |w| < 2^23, |d| < 2^8
  };
  // the same with the background total as the addend: h = bgtot + ...
  auto first_span = [&](uint32_t sp, int (&h)[3]) __attribute__((always_inline)) {
    const int a = sp & 1023, b = (sp >> 10) & 1023;
    const int dpk = __builtin_amdgcn_readlane((int)dpk_reg, (int)(sp >> 20));
    // (the three signed 10-bit fields: shifted up as unsigned -- a signed shift into the sign bit is undefined before C++20 --,
    // then down arithmetically: the same two instructions per field)
    const uint32_t dpu = (uint32_t)dpk;
    const int d0 = (int)(dpu << 22) >> 22, d1 = (int)(dpu << 12) >> 22, d2 = (int)(dpu << 2) >> 22;
    const int w = pbase[med3_su(b, hlo, hhi)] - pbase[med3_su(a, hlo, hhi)];
    // explicit three-operand mads: written in C the compiler tail-merges this block with add_span
    // and pays three v_mov per canvas row to seed h with the background total
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(h[0]) : "v"(w), "s"(d0), "v"(bgtot0));
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(h[1]) : "v"(w), "s"(d1), "v"(bgtot1));
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(h[2]) : "v"(w), "s"(d2), "v"(bgtot2));
  };
  swb_u4 rec = *reinterpret_cast<cptr<swb_u4>>(runs + uo);       // { row | rows-1 << 16 | spans << 24, span 0, span 1, span 2 }
  int h[3] = {0, 0, 0};                                // the horizontal pass of the last run that carried spans, clipped
  bool more = true;
  while (more) {
#pragma unroll
    for (int k = 0; k < VS; ++k) {                     // output row r_first accumulates in slot k
      // the runs left in this row's window (a run never extends past the row that ends an output row)
      while ((int)(rec.x & 0xffffu) <= next_end) {
        const uint32_t ro = (rec.x & 0xffffu) << 5;                                      // SWB_VSLOTS * 4 bytes per table row
        const uint32_t eo = ro + ((rec.x >> 11) & (63u << 5));
        swb_i8 ps = *reinterpret_cast<cptr<swb_i8>>(vpfx + ro);
        swb_i8 pe = *reinterpret_cast<cptr<swb_i8>>(vpfx + eo + 32);
        SWB_LOADED_HERE(ps); SWB_LOADED_HERE(pe);
        // horizontal pass of the run's row (Resample.c ImagingResampleHorizontal_8bpc).  The first span starts from
        // the background total, so h needs no separate initialisation; an absent span is empty (0..0).
        // A continuation run (SWB_RUN_CONTINUES: one unit) keeps the h of the run before it.  (Regions of if-then only: an
        // if-else on the kind of run -- one span / several / continuation -- comes out of the compiler with a flag register
        // and two more branches on the path of the one-span run.)
        const uint32_t u0 = uo;
        uo += 8u;                                                                        // a run of up to one span, a continuation: one unit
        if (__builtin_expect(!(rec.x & SWB_RUN_CONTINUES), 1)) {
          const int ns = (int)(rec.x >> 24);
          first_span(rec.y, h);
          if (ns >= 2) {
            add_span(rec.z, h);
            uo += (uint32_t)(ns >> 1) << 3;                                              // run_units(ns) * 8 in all
            if (ns >= 3) {
              add_span(rec.w, h);
              for (int m = SWB_REG_SPANS; m < ns; ++m)
                add_span(*reinterpret_cast<cptr<uint32_t>>(runs + u0 + 8u * (uint32_t)(2 + ((m - 3) >> 1)) + 4u * (uint32_t)((m - 3) & 1)), h);
            }
          }
          h[0] = clip8_fix(h[0]); h[1] = clip8_fix(h[1]); h[2] = clip8_fix(h[2]);
        }
        rec = *reinterpret_cast<cptr<swb_u4>>(runs + uo);
        // vertical pass contribution (Resample.c ImagingResampleVertical_8bpc): coefficient sums of the run's rows
#pragma unroll
        for (int j = 0; j < VS; ++j) {
          const int kv = pe[j] - ps[j];
          acc[0][j] += __mul24(kv, h[0]); acc[1][j] += __mul24(kv, h[1]); acc[2][j] += __mul24(kv, h[2]);
        }
      }
      // finish output row r_first: clip, pack, store; rows above the band only free their slot.  (Written so that the slot's
      // accumulators leave this block as constants on every path -- an untouched slot holds its restart value already -- and the
      // store takes a 32-bit byte offset from a uniform base: the round-5 form, which kept them on the untouched path and indexed
      // a dword pointer, cost 10 register moves and address computations per finished row, a tenth of the kernel's vector
      // instructions on the headline scene.)
      {
        const bool untouched = black && mark[k] == uo;
        if (r_first >= o_lo) {
          uint32_t dw = 0u;
          if (!untouched) {
            // px = c0 | c1 << 8 | c2 << 16 in two shift-and-or instructions (written in C: two shifts and a three-input or);
            // the DPP move with bound_ctrl, so that no register has to be zeroed for lanes the move does not reach (there are none)
            const uint32_t c0 = (uint32_t)clip8_fix(acc[0][k]), c1 = (uint32_t)clip8_fix(acc[1][k]), c2 = (uint32_t)clip8_fix(acc[2][k]);
            uint32_t px01, px;
            SWB_LSHL_OR(px01, c1, 8, c0);
            SWB_LSHL_OR(px, c2, 16, px01);
            const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)px, 0xF9, 0xf, 0xf, true);    // quad_perm:[1,2,3,3]
            dw = __builtin_amdgcn_perm(nb, px, pack_sel);
          }
          if (pack_store) *reinterpret_cast<uint32_t*>(frame_bytes + dst_off) = dw;
          dst_off -= row_bytes;
        }
        acc[0][k] = SWB_HALF; acc[1][k] = SWB_HALF; acc[2][k] = SWB_HALF;
        mark[k] = uo;
      }
      ++r_first;
      next_end = next_end2;
      next_end2 = as_const(p.v_end)[r_first + 1];
      if (prio > 0 && ((u_end - uo) >> prio_shift) < (uint32_t)prio) {      // (rare: at most three times per wave)
        --prio;
        if (prio == 2) __builtin_amdgcn_s_setprio(2);
        else if (prio == 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      if (r_first >= o_hi) { more = false; break; }
    }
  }
  // Fill (SWB_RHDR_FRAME = 1): the rectangle this wave has just written goes into the cache as well.  A tail, not a second store in
  // the finished-row block: the loop above is the parent's, instruction for instruction, for the waves that only resample.  The
  // dwords a lane copies were stored by other lanes of this wave: a workgroup-scope release / acquire pair lies between.
  if (frame_mode == 1u) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    copy_frame_rect(p.obs + frame_off, p.frame_cache + frame_off, rect_row_bytes, rect_seg_bytes, o_hi - o_lo, p.obs_aligned16 != 0);
  }
  if (p.frame_stats && l == 0) atomicAdd(&p.frame_stats[4], (unsigned long long)((uint32_t)__builtin_amdgcn_s_memtime() - cycles0));
}

#ifndef SWB_WIDE_TU
// --------------------------------------------------------------------------------------------
// Kernel 2 of a step when anti_aliasing = 1, "fill": pil_renderer.py:84 resizes to the same size, i.e. copies, so
// the canvas is the image.  One (environment, column group, band of rows) per wave, lanes = columns: rows no run
// covers are background, a run's row is built once (packed in registers as in the resample kernel) and stored
// for each of its rows.  Every pixel is written exactly once.
// --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SWB_WAVE* SWB_RS_WAVES_PER_BLOCK, SWB_RS_WAVES_PER_SIMD)
swb_fill_kernel(const swb_params p) {
  const int wave = rfl(threadIdx.x >> 6);
  const int l = lane_id();
  const int task = blockIdx.x * SWB_RS_WAVES_PER_BLOCK + wave;
  int band = blockIdx.y;
  // consecutive blocks of a shard take tasks (environment, column group[, band]) of decreasing cost: the eight waves of a SIMD get
  // one of every octile.  (Without cost ordering: blockIdx.z is the column group.)
  int env = task < p.N ? task : -1, g = blockIdx.z;
  if (p.cost_cnt) {
    env = cost_ordered_env(p, p.parity, (int)(blockIdx.x & (SWB_COST_SHARDS - 1)),
                           dealt_block(p, (int)(blockIdx.x >> 3), (int)(gridDim.x >> 3)) * SWB_RS_WAVES_PER_BLOCK + wave);
    env = rfl(env);
    if (env >= 0) {
      if (p.band_tasks) band = (env >> 26) & 7;
      g = (env >> 24) & 3; env &= 0xffffff;
    }
    if (blockIdx.y == 0) cost_housekeeping(p, (int)blockIdx.x, wave);
  }
  if (env < 0) return;
  const int y_lo = as_const(p.band_lo)[band], y_hi = as_const(p.band_lo)[band + 1];
  if (y_lo >= y_hi) return;
  cptr<uint32_t> hdr = as_const(p.rhdr) + (size_t)env * SWB_RHDR_DWORDS;
  const uint32_t rgb_reg = (l < SWB_TUNED_SPRITES) ? p.rhdr[(size_t)env * SWB_RHDR_DWORDS + SWB_TUNED_SPRITES + l] : 0u;
  const int n_units = (int)hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE];       // (positions: see swb_params::run_cap)
  int u = (int)hdr[SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE + 1 + band];
  cptr<uint32_t> runs = as_const(p.runs) + ((size_t)env * p.ncg + g) * p.run_cap * 2;
  const int x = 64 * g + l;
  const int nd = (p.Wo * 3) >> 2;
  unsigned char* const frame_bytes = p.obs + (size_t)env * p.Wo * p.Ho * 3;
  const uint32_t row_bytes = 4u * (uint32_t)nd;
  const uint32_t pack_sel = ((l & 3) == 0) ? 0x04020100u : (((l & 3) == 1) ? 0x05040201u : 0x06050402u);
  const bool pack_store = ((l & 3) != 3) && (x < p.Wo);
  uint32_t dst_off = 4u * (uint32_t)((p.Ho - 1 - y_lo) * nd + 48 * g + 3 * (l >> 2) + (l & 3));   // in bytes; np.flipud :90: canvas row y is image row Ho-1-y
  auto pack = [&](uint32_t col) __attribute__((always_inline)) {
    const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)col, 0xF9, 0xf, 0xf, false);   // quad_perm:[1,2,3,3]
    return __builtin_amdgcn_perm(nb, col, pack_sel);
  };
  const uint32_t bg_dw = pack(p.bg);
  int y = y_lo;
  while (y < y_hi) {
    uint32_t hd = 0u, s0 = 0u, s1 = 0u, s2 = 0u;
    int r = y_hi;
    if (u < n_units) {
      hd = runs[2 * u]; s0 = runs[2 * u + 1]; s1 = runs[2 * u + 2]; s2 = runs[2 * u + 3];
      r = min((int)(hd & 0xffffu), y_hi);
    }
    for (; y < r; ++y) { if (pack_store) *reinterpret_cast<uint32_t*>(frame_bytes + dst_off) = bg_dw; dst_off -= row_bytes; }       // rows without spans
    if (y >= y_hi) break;
    const int len = (int)((hd >> 16) & 63u) + 1, ns = (int)(hd >> 24);
    uint32_t col = p.bg;
    auto paint = [&](uint32_t sp) __attribute__((always_inline)) {
      const int a = sp & 1023, b = (sp >> 10) & 1023;
      const uint32_t rgb = (uint32_t)__builtin_amdgcn_readlane((int)rgb_reg, (int)(sp >> 20));
      if (x >= a && x < b) col = rgb;
    };
    paint(s0);
    if (ns >= 2) {
      paint(s1);
      if (ns >= 3) {
        paint(s2);
        for (int m = SWB_REG_SPANS; m < ns; ++m) paint(runs[2 * (u + 2 + ((m - 3) >> 1)) + ((m - 3) & 1)]);
      }
    }
    const uint32_t dw = pack(col);
    const int stop = min(y + len, y_hi);
    for (; y < stop; ++y) { if (pack_store) *reinterpret_cast<uint32_t*>(frame_bytes + dst_off) = dw; dst_off -= row_bytes; }
    u += run_units(ns);
  }
}


// The five scalars of one environment, gathered into one 20-byte record (swb_get_env_state: one copy instead of five).
__global__ void swb_env_state_kernel(const swb_params p, int env, int32_t* out5) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    out5[0] = p.nspr[env]; out5[1] = p.entry[env]; out5[2] = p.step_count[env]; out5[3] = p.episode[env];
    out5[4] = (int32_t)p.reset_next[env];
  }
}

// --------------------------------------------------------------------------------------------
// SpriteFactors observation (renderers/handcrafted.py:29-82): one thread per (env, sprite).
// --------------------------------------------------------------------------------------------
__global__ void swb_factors_kernel(const swb_params p, double* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.N * p.S) return;
  const int env = idx / p.S, s = idx - env * p.S;
  double* o = out + (size_t)idx * 10;
  const int n = p.nspr[env];
  if (s >= n) {
    for (int k = 0; k < 10; ++k) o[k] = 0.0;
    return;
  }
  const size_t pe = (size_t)p.entry[env] * p.S + s;
  const bool ov = p.ov_flag && p.ov_flag[env];          // sprite.py:152-175 setters were applied to this episode
  o[0] = p.x[idx]; o[1] = p.y[idx];
  o[2] = (double)((ov ? p.ov_shape[idx] : p.p_shape[pe]) + 1);        // constants.ShapeType value
  o[3] = ov ? p.ov_angle[idx] : (p.p_angle ? p.p_angle[pe] : 0.0);
  o[4] = ov ? p.ov_scale[idx] : p.p_scale[pe];
  o[5] = p.p_color ? p.p_color[3 * pe] : 0.0;
  o[6] = p.p_color ? p.p_color[3 * pe + 1] : 0.0;
  o[7] = p.p_color ? p.p_color[3 * pe + 2] : 0.0;
  o[8] = p.p_xv[pe]; o[9] = p.p_yv[pe];
}

// --------------------------------------------------------------------------------------------
// Large-frame path: canvases wider than the widest cover build (640 px) and images wider than SWB_MAX_CG column groups.
// The cover kernel runs its state phase only (obs = NULL); then
//   swb_lf_raster_kernel    one workgroup of SWB_LF_WAVES waves per (environment, block of canvas rows).  The workgroup
//                           builds every sprite's Pillow edges once (LDS); a wave then takes one canvas row at a time:
//                           polygon_generic of every sprite, back to front, paints sprite ids into a byte row in LDS, and
//                           the horizontal LANCZOS pass walks the constant-colour spans of the row inside each output
//                           column's window: colour x (prefix[end] - prefix[start]), exact integers.  uint8 result ->
//                           scratch [envs of the chunk][Hc][Wo][3].  anti_aliasing = 1: the row is the image row, stored
//                           flipped straight into obs.
//   swb_lf_vertical_kernel  lanes = 4-byte words of an output row: the vertical pass over the scratch rows, flipped into obs.
// Arithmetic is oracle/sw_oracle.c's draw_polygon / resample_lanczos, operation for operation.
// --------------------------------------------------------------------------------------------
#define SWB_LF_WAVES 4
#define SWB_LF_MAX_CROSS (2 * SWB_MAX_SHAPE_VERTS)   // crossings of one sprite on one row (an edge may count twice)

struct swb_lf_args {
  const int32_t* hb;           // [Wo][2] horizontal windows (xmin, count)
  const int32_t* hpo;          // [Wo] offset of output column o's prefix sums in hp
  const int32_t* hp;           // per output column: count + 1 prefix sums of its coefficients
  const int32_t* vb;           // [Ho][2] vertical windows (ymin, count)
  const int32_t* vk;           // [Ho][vks] vertical coefficients
  int32_t vks;
  int32_t e0, ne;              // environments [e0, e0 + ne) of this chunk
  int32_t rows_per_block;      // canvas rows per workgroup of the raster kernel
  int32_t max_verts_env;       // vertex capacity of the workgroup's LDS tables (swb_params::max_edges)
  int32_t row_bytes;           // LDS bytes of a wave's row buffer (Wc rounded up)
  int32_t mask_words;          // ... of its span-boundary bit mask (Wc / 32 + 1: bit Wc is a sentinel)
  uint8_t* tmp;                // [ne][Hc][Wo][3] horizontal pass (anti_aliasing > 1)
};

struct swb_lf_xy { int32_t x, y; };

struct swb_lf_edge {           // Draw.c Edge (x0, y0 as given; ymin > ymax: not an edge)
  int32_t x0, y0, xmin, xmax, ymin, ymax;
  float dx;
  int32_t pad;
};

struct swb_lf_block {          // workgroup-shared head of the raster kernel's LDS
  uint32_t col[SWB_MAX_SPRITES + 1];   // 0: background, s + 1: sprite s
  int32_t n, vtotal, err, pad0;
  int32_t voff[SWB_MAX_SPRITES], nv[SWB_MAX_SPRITES], so[SWB_MAX_SPRITES];
  int32_t ymin[SWB_MAX_SPRITES], ymax[SWB_MAX_SPRITES], ymaxc[SWB_MAX_SPRITES];
  double px[SWB_MAX_SPRITES], py[SWB_MAX_SPRITES], sc[SWB_MAX_SPRITES], ca[SWB_MAX_SPRITES], sa[SWB_MAX_SPRITES];
};

__host__ __device__ __forceinline__ size_t swb_lf_head_bytes(int max_verts) {
  return ((sizeof(swb_lf_block) + 15) & ~(size_t)15) + (size_t)max_verts * 8 + (size_t)max_verts * sizeof(swb_lf_edge);
}

// Index of the lowest set bit of a non-zero 64-bit mask.
__device__ __forceinline__ int swb_lf_first_lane(unsigned long long m) {
  const uint32_t lo = (uint32_t)m;
  return lo ? __ffs((int)lo) - 1 : 31 + __ffs((int)(uint32_t)(m >> 32));
}

// Draw.c hline clipping: [x0, x1] on a row of W pixels; false when nothing is drawn.
__device__ __forceinline__ bool swb_lf_clip(int& x0, int& x1, int W) {
  if (x0 < 0) x0 = 0;
  else if (x0 >= W) return false;
  if (x1 < 0) return false;
  if (x1 >= W) x1 = W - 1;
  return x0 <= x1;
}

__global__ void __launch_bounds__(SWB_WAVE * SWB_LF_WAVES)
swb_lf_raster_kernel(const swb_params p, const swb_lf_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, l = lane_id(), wave = rfl(t >> 6);
  const int env = a.e0 + (int)blockIdx.y, S = p.S;
  const int Wc = p.Wc, Hc = p.Hc;
  swb_lf_block* B = reinterpret_cast<swb_lf_block*>(smem);
  swb_lf_xy* verts = reinterpret_cast<swb_lf_xy*>(smem + ((sizeof(swb_lf_block) + 15) & ~(size_t)15));
  swb_lf_edge* edges = reinterpret_cast<swb_lf_edge*>(verts + a.max_verts_env);
  unsigned char* wbase = smem + swb_lf_head_bytes(a.max_verts_env) +
                         (size_t)wave * (a.row_bytes + 4 * a.mask_words + 2 * 4 * SWB_LF_MAX_CROSS);
  unsigned char* row = wbase;                                            // sprite id + 1 per canvas pixel (0: background)
  uint32_t* bmask = reinterpret_cast<uint32_t*>(wbase + a.row_bytes);  // bit x: pixel x starts a span (x = Wc: sentinel)
  float* xs = reinterpret_cast<float*>(bmask + a.mask_words);          // crossings of a row, in edge order
  float* srt = xs + SWB_LF_MAX_CROSS;                                  // ... sorted

  // ---- the environment's sprites (the state the cover kernel's state phase left): pool entry or setter overrides
  const bool ov = p.ov_flag != nullptr && p.ov_flag[env] != 0;
  const int n = p.nspr[env];
  const size_t pe = (size_t)p.entry[env] * S;
  if (t == 0) { B->col[0] = p.bg; B->n = n; B->err = 0; }
  if (t < n) {
    int sh = ov ? p.ov_shape[(size_t)env * S + t] : p.p_shape[pe + t];
    sh = min(max(sh, 0), SWB_MAX_SHAPES - 1);
    B->so[t] = p.shape_off[sh];
    B->nv[t] = p.shape_off[sh + 1] - p.shape_off[sh];
    B->col[t + 1] = p.p_rgb[pe + t];
    B->px[t] = p.x[(size_t)env * S + t]; B->py[t] = p.y[(size_t)env * S + t];
    B->sc[t] = p.p_scale[pe + t]; B->ca[t] = p.p_ca[pe + t]; B->sa[t] = p.p_sa[pe + t];
  }
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int s = 0; s < n; ++s) {
      if (tot + B->nv[s] > a.max_verts_env) { B->n = s; B->err = SWB_ENV_ERR_SPAN_OVERFLOW; break; }   // (cannot happen: sized by the pool)
      B->voff[s] = tot;
      tot += B->nv[s];
    }
    B->vtotal = tot;
  }
  __syncthreads();
  const int ns = B->n, vtotal = B->vtotal;
  // vertices -> canvas ints: sprite.py:131-133 translate, then (int)(canvas size * v) (C truncation)
  bool all_fit = true;
  for (int k = t; k < vtotal; k += blockDim.x) {
    int sid = 0;
    for (int s = 1; s < ns; ++s) if (k >= B->voff[s]) sid = s;
    const int i = k - B->voff[sid];
    double cx, cy;
    if (ov) {
      const double* q = p.ov_cpath + (((size_t)env * S + sid) * SWB_MAX_SHAPE_VERTS + i) * 2;
      cx = q[0]; cy = q[1];
    } else {
      centered_vertex(p, B->so[sid], i, B->sc[sid], B->ca[sid], B->sa[sid], cx, cy);
    }
    const double vx = __dadd_rn(__dadd_rn(__dmul_rn(1.0, cx), __dmul_rn(0.0, cy)), B->px[sid]);
    const double vy = __dadd_rn(__dadd_rn(__dmul_rn(0.0, cx), __dmul_rn(1.0, cy)), B->py[sid]);
    // (decided on the doubles, as in the cover kernel's P1b: within +-2^24 the difference of two coordinates fits an int and
    // is exact as a float; a vertex beyond that, or not finite, is flagged and stored as 0)
    const double fx = __dmul_rn((double)Wc, vx), fy = __dmul_rn((double)Hc, vy);
    const bool fits = fabs(fx) < SWB_LF_COORD_LIMIT + 1.0 && fabs(fy) < SWB_LF_COORD_LIMIT + 1.0;
    all_fit = all_fit && fits;
    verts[k] = swb_lf_xy{fits ? (int)fx : 0, fits ? (int)fy : 0};
  }
  if (!all_fit) B->err = SWB_ENV_ERR_SPAN_OVERFLOW;      // (every writer stores the same value)
  __syncthreads();
  // Draw.c add_edge: edge i joins vertex i and i + 1; the closing edge only if the last vertex differs from the first
  for (int k = t; k < vtotal; k += blockDim.x) {
    int sid = 0;
    for (int s = 1; s < ns; ++s) if (k >= B->voff[s]) sid = s;
    const int vb = B->voff[sid], nv = B->nv[sid], i = k - vb;
    const swb_lf_xy f = verts[vb], g = verts[vb + nv - 1];
    const int ne = (g.x != f.x || g.y != f.y) ? nv : nv - 1;
    swb_lf_edge e;
    e.pad = 0;
    if (i < ne) {
      const swb_lf_xy v0 = verts[k], v1 = verts[(i + 1 == nv) ? vb : k + 1];
      e.x0 = v0.x; e.y0 = v0.y;
      e.xmin = min(v0.x, v1.x); e.xmax = max(v0.x, v1.x);
      e.ymin = min(v0.y, v1.y); e.ymax = max(v0.y, v1.y);
      e.dx = (v0.y == v1.y) ? 0.0f : __fdiv_rn((float)(v1.x - v0.x), (float)(v1.y - v0.y));
    } else {
      e.x0 = e.y0 = e.xmin = e.xmax = 0; e.ymin = 1; e.ymax = 0; e.dx = 0.0f;
    }
    edges[k] = e;
  }
  __syncthreads();
  // rows a sprite's scan visits: Draw.c starts ymin at ysize - 1 and ymax at 0, clamps ymin to 0 and ymax to ysize
  // (the rows themselves are those with an edge on them: ymin only starts the loop, ymax also decides the duplicated crossing)
  if (t < ns) {
    int lo = 0x7fffffff, hi = -0x7fffffff;
    for (int k = B->voff[t]; k < B->voff[t] + B->nv[t]; ++k) {
      const swb_lf_edge e = edges[k];
      if (e.ymin > e.ymax) continue;
      lo = min(lo, e.ymin); hi = max(hi, e.ymax);
    }
    B->ymin[t] = lo; B->ymax[t] = hi;
    B->ymaxc[t] = min(max(hi, 0), Hc);
  }
  __syncthreads();
  if (t == 0 && blockIdx.x == 0 && B->err && p.error) p.error[env] |= (uint8_t)B->err;

  const int y_lo = (int)blockIdx.x * a.rows_per_block, y_hi = min(y_lo + a.rows_per_block, Hc);
  const int Wo = p.Wo, Ho = p.Ho;
  const unsigned long long below = (1ull << l) - 1ull;
  for (int y = y_lo + wave; y < y_hi; y += SWB_LF_WAVES) {
    // canvas.paste(bg)
    for (int w = l; w < (a.row_bytes >> 2); w += SWB_WAVE) reinterpret_cast<uint32_t*>(row)[w] = 0u;
    wave_sync();
    for (int s = 0; s < ns; ++s) {                            // back to front (pil_renderer.py:80-83)
      if (y < B->ymin[s] || y > B->ymax[s]) continue;         // (wave-uniform) no edge of the sprite on this row
      const int eo = B->voff[s], ne = B->nv[s], ymaxc = B->ymaxc[s];
      const unsigned char id = (unsigned char)(s + 1);
      // lane i = edge i of the sprite (at most SWB_MAX_SHAPE_VERTS)
      swb_lf_edge cur;
      cur.ymin = 1; cur.ymax = 0; cur.dx = 0.0f; cur.x0 = cur.y0 = cur.xmin = cur.xmax = 0;
      if (l < ne) cur = edges[eo + l];
      const bool horiz = cur.ymin == cur.ymax;
      int hx0 = cur.xmin, hx1 = cur.xmax;
      const bool hline_l = horiz && y == cur.ymin && swb_lf_clip(hx0, hx1, Wc);   // horizontal edges: drawn as they are
      int cnt = 0;
      float xx = 0.0f;
      if (!horiz && y >= cur.ymin && y <= cur.ymax) {
        xx = pil_cross(y, cur.y0, cur.dx, cur.x0);
        cnt = 1;
        if (y == cur.ymax && y < ymaxc) {
          cnt = 2;                                            // "needed to draw consistent polygons"
        } else if (cur.dx != 0.0f && (y == cur.ymin || y == cur.ymax)) {
          // connect discontiguous corners: the first EARLIER edge of the table that also ends on this row
          const int adj = (y == cur.ymax) ? y - 1 : y + 1;
          for (int k = 0; k < l; ++k) {
            const swb_lf_edge o = edges[eo + k];
            if (o.ymin >= o.ymax) continue;                    // (horizontal edges are not in the table)
            if ((y != o.ymin && y != o.ymax) || o.dx == 0.0f) continue;
            if (roundf(xx) != roundf(pil_cross(y, o.y0, o.dx, o.x0))) continue;
            if (adj < o.ymin || adj > o.ymax) continue;
            const float ca = pil_cross(adj, cur.y0, cur.dx, cur.x0);
            const float cb = pil_cross(adj, o.y0, o.dx, o.x0);
            if (xx > __fadd_rn(ca, 1.0f) && xx > __fadd_rn(cb, 1.0f))
              xx = __fadd_rn(roundf(fmaxf(ca, cb)), 1.0f);
            else if (xx < __fsub_rn(ca, 1.0f) && xx < __fsub_rn(cb, 1.0f))
              xx = __fsub_rn(roundf(fminf(ca, cb)), 1.0f);
            break;
          }
        }
      }
      // crossings in edge order -> LDS, sorted by rank (ties keep their order: equal values are interchangeable)
      const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(cnt == 2);
      const int pos = __popcll(m1 & below) + __popcll(m2 & below);
      const int j = __popcll(m1) + __popcll(m2);
      if (cnt >= 1) xs[pos] = xx;
      if (cnt == 2) xs[pos + 1] = xx;
      wave_sync();
      if (cnt >= 1) {
        int r = 0;
        for (int m = 0; m < j; ++m) {
          const float v = xs[m];
          r += (v < xx || (v == xx && m < pos)) ? 1 : 0;
        }
        srt[r] = xx;
        if (cnt == 2) srt[r + 1] = xx;
      }
      wave_sync();
      // pairs: hline(ROUND_UP(xx[2i]), y, ROUND_DOWN(xx[2i + 1]))
      int fx0 = 0, fx1 = -1;
      bool fill_l = false;
      if (2 * l + 1 < j) {
        fx0 = pil_round_up(srt[2 * l]);
        fx1 = pil_round_down(srt[2 * l + 1]);
        fill_l = swb_lf_clip(fx0, fx1, Wc);
      }
      for (int pass = 0; pass < 2; ++pass) {
        unsigned long long m = __ballot(pass == 0 ? hline_l : fill_l);
        while (m) {
          const int src = swb_lf_first_lane(m);
          const int x0 = __builtin_amdgcn_readlane(pass == 0 ? hx0 : fx0, src);
          const int x1 = __builtin_amdgcn_readlane(pass == 0 ? hx1 : fx1, src);
          for (int x = x0 + l; x <= x1; x += SWB_WAVE) row[x] = id;
          m &= m - 1ull;
        }
      }
      wave_sync();
    }
    if (p.AA == 1) {
      // the canvas is the image (pil_renderer.py:84 resizes to the same size): np.flipud into obs, 4-byte words
      const int nd = (Wo * 3) >> 2;
      uint32_t* dst = reinterpret_cast<uint32_t*>(p.obs + ((size_t)env * Ho + (size_t)(Ho - 1 - y)) * (size_t)Wo * 3);
      for (int d = l; d < nd; d += SWB_WAVE) {
        uint32_t w = 0u;
        for (int b = 0; b < 4; ++b) {
          const int byte = 4 * d + b, px = byte / 3, ch = byte - 3 * px;
          w |= ((B->col[row[px]] >> (8 * ch)) & 255u) << (8 * b);
        }
        dst[d] = w;
      }
      wave_sync();
      continue;
    }
    // span starts of the row (bit x: pixel x differs from pixel x - 1; bit Wc ends the last span)
    for (int w = l; w < a.mask_words; w += SWB_WAVE) {
      uint32_t bits = 0u;
      const int xb = 32 * w;
      int prev = (xb >= 1 && xb - 1 < Wc) ? row[xb - 1] : -1;
      for (int b = 0; b < 32; ++b) {
        const int x = xb + b;
        if (x > Wc) break;
        if (x == Wc) { bits |= 1u << b; break; }
        const int c = row[x];
        if (x >= 1 && c != prev) bits |= 1u << b;
        prev = c;
      }
      bmask[w] = bits;
    }
    wave_sync();
    // horizontal pass (Resample.c, 8 bpc): output column o sums colour x coefficient over the spans inside its window
    uint8_t* out_row = a.tmp + ((size_t)(env - a.e0) * Hc + (size_t)y) * (size_t)Wo * 3;
    for (int o = l; o < Wo; o += SWB_WAVE) {
      const int xmin = as_const(a.hb)[2 * o], xend = xmin + as_const(a.hb)[2 * o + 1];
      cptr<int32_t> pf = as_const(a.hp) + as_const(a.hpo)[o];
      int s0 = SWB_HALF, s1 = SWB_HALF, s2 = SWB_HALF;
      int x = xmin, wlo = 0;
      while (x < xend) {
        // next span start after x (the sentinel at Wc bounds the search)
        int wi = (x + 1) >> 5;
        uint32_t bits = bmask[wi] & (0xffffffffu << ((x + 1) & 31));
        while (bits == 0u && 32 * (wi + 1) < xend) bits = bmask[++wi];
        int nx = bits ? 32 * wi + __ffs((int)bits) - 1 : xend;
        nx = min(nx, xend);
        const int whi = pf[nx - xmin];
        const int k = whi - wlo;
        const uint32_t c = B->col[row[x]];
        s0 += (int)(c & 255u) * k; s1 += (int)((c >> 8) & 255u) * k; s2 += (int)((c >> 16) & 255u) * k;
        wlo = whi;
        x = nx;
      }
      out_row[3 * o] = (uint8_t)clip8_fix(s0);
      out_row[3 * o + 1] = (uint8_t)clip8_fix(s1);
      out_row[3 * o + 2] = (uint8_t)clip8_fix(s2);
    }
    wave_sync();
  }
}

// Vertical pass + np.flipud: lanes = 4-byte words of output row r (wave-uniform), its window of scratch rows.
__global__ void __launch_bounds__(SWB_WAVE * SWB_LF_WAVES)
swb_lf_vertical_kernel(const swb_params p, const swb_lf_args a) {
  const int wave = rfl(threadIdx.x >> 6);
  const int r = (int)blockIdx.y * SWB_LF_WAVES + wave;
  const int env = a.e0 + (int)blockIdx.z;
  const int nd = (p.Wo * 3) >> 2;
  const int d = (int)blockIdx.x * SWB_WAVE + lane_id();
  if (r >= p.Ho || d >= nd) return;
  const int ymin = as_const(a.vb)[2 * r], cnt = as_const(a.vb)[2 * r + 1];
  cptr<int32_t> k = as_const(a.vk) + (size_t)r * a.vks;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tmp + (size_t)(env - a.e0) * p.Hc * (size_t)p.Wo * 3) +
                        (size_t)ymin * nd + d;
  int s0 = SWB_HALF, s1 = SWB_HALF, s2 = SWB_HALF, s3 = SWB_HALF;
  for (int i = 0; i < cnt; ++i) {
    const uint32_t w = src[(size_t)i * nd];
    const int c = k[i];
    s0 += (int)(w & 255u) * c; s1 += (int)((w >> 8) & 255u) * c;
    s2 += (int)((w >> 16) & 255u) * c; s3 += (int)(w >> 24) * c;
  }
  const uint32_t out = (uint32_t)clip8_fix(s0) | ((uint32_t)clip8_fix(s1) << 8) | ((uint32_t)clip8_fix(s2) << 16) |
                       ((uint32_t)clip8_fix(s3) << 24);
  reinterpret_cast<uint32_t*>(p.obs + ((size_t)env * p.Ho + (size_t)(p.Ho - 1 - r)) * (size_t)p.Wo * 3)[d] = out;
}

#endif  // SWB_WIDE_TU

// --------------------------------------------------------------------------------------------
// Many-sprite path (handles of more than SWB_TUNED_SPRITES sprites, up to SWB_MAX_SPRITES = one lane per sprite): the
// state phase of a step -- the three shared pieces the cover kernel's P0 runs (load_env_state, act_and_move, finish_step) -- in a
// kernel of its own, one wave per environment; the frame is then rendered by the large-frame kernels above.
// What is its own: the scan of vertex offsets and the centred paths of the whole scene are not needed (P1 is not run here), so
// a hit test builds the centred path of the one sprite it visits on the fly (lanes = vertices, <= SWB_MAX_SHAPE_VERTS), and
// the LDS is a wide task_scratch and one path, about 6 KB per wave whatever the scene.
// --------------------------------------------------------------------------------------------
struct swb_ms_lds {
  task_scratch_t<SWB_MAX_SPRITES> ts;
  double2 path[SWB_MAX_SHAPE_VERTS];                    // centred path of the sprite a hit test visits
};
static_assert(SWB_MAX_SPRITES <= SWB_WAVE && SWB_MAX_SHAPE_VERTS <= SWB_WAVE, "one lane per sprite / per vertex");

#endif                     // ---- SWB_SETS_PASS
#ifdef SWB_SETS_PASS
__global__ void __launch_bounds__(SWB_WAVE)
swb_ms_state_sets_kernel(const swb_params p) {
  constexpr bool OV = true, SETS = true;
#else
template <bool OV>
__global__ void __launch_bounds__(SWB_WAVE)
swb_ms_state_kernel(const swb_params p) {
  constexpr bool SETS = false;
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int l = lane_id();
  const int env = blockIdx.x;
  swb_ms_lds* M = reinterpret_cast<swb_ms_lds*>(smem);
  task_scratch_t<SWB_MAX_SPRITES>* tscratch = &M->ts;
  double2* cpath = M->path;
  const uint32_t task_rec_l = load_task_record(p, env);
  env_state es = load_env_state<OV>(p, env, tscratch);
  park_task_record(p, task_rec_l, tscratch);
  // sprite.py:113-115 contains_point of sprite s2 (wave-uniform): its centred path into LDS, lanes = vertices, then the
  // even-odd test of contains_point_wave -- the values P1a of the cover kernel computes for the same sprite
  auto hit = [&](int s2, double tx, double ty) __attribute__((always_inline)) {
    const int nv = __builtin_amdgcn_readlane(es.nv_l, s2), so = __builtin_amdgcn_readlane(es.so_l, s2);
    const double sc = readlane_d(es.scale_l, s2), ca = readlane_d(es.ca_l, s2), sa = readlane_d(es.sa_l, s2);
    wave_sync();                                        // (the previous sprite's test has read the path)
    if (l < nv) {
      double cx, cy;
      bool from_table = true;
      if constexpr (OV) {
        if (es.ov) {                                    // the path the setters left (host arithmetic, swb.hip)
          const double* q = p.ov_cpath + (((size_t)env * p.S + s2) * SWB_MAX_SHAPE_VERTS + l) * 2;
          cx = q[0]; cy = q[1];
          from_table = false;
        }
      }
      if (from_table) centered_vertex(p, so, l, sc, ca, sa, cx, cy);
      cpath[l] = make_double2(cx, cy);
    }
    wave_sync();
    return contains_point_wave(cpath, nv, tx, ty);
  };
  const step_cost sc = act_and_move(p, env, es, hit);
  if (p.render_only != 1 && es.active) {
    const uint32_t err = finish_step<OV, true, SETS>(p, env, es, sc, tscratch);
    if (l == 0 && p.error && err) p.error[env] |= (uint8_t)err;         // sticky: the caller clears
  }
}
#ifndef SWB_SETS_PASS      // ---- (to the end of the file)

// The kernels of handles with task sets live in swb_wide.hip's code object: the one of swb.hip stays what it was.
__global__ void swb_ms_state_sets_kernel(const swb_params p);
__global__ void swb_env_task_sets_kernel(const int32_t* entry, const uint8_t* set_of_entry, int32_t* out, int N, int entries);
#ifdef SWB_WIDE_TU
#define SWB_SETS_PASS 1
#include "swb_kernels.hip.inc"
#undef SWB_SETS_PASS
// swb_env_task_sets: the set of the entry every environment is in (entries: the pool's; an entry outside it -- none is ever
// written -- reads entry 0)
__global__ void __launch_bounds__(256)
swb_env_task_sets_kernel(const int32_t* entry, const uint8_t* set_of_entry, int32_t* out, int N, int entries) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int e = entry[n];
  out[n] = (int32_t)set_of_entry[(e >= 0 && e < entries) ? e : 0];
}
#endif

// --------------------------------------------------------------------------------------------
// Rollouts (swb_rollout): what would M candidate action sequences of K steps earn from where every environment is NOW?
// N * M virtual environments (v = n * M + m) step K times on a private copy of the state; the live state is only read.
//   swb_rollout_fork_kernel  copies the live per-environment state into the scratch arrays of the virtual environments,
//                            replicates pool_base / pool_len (one thread per (v, sprite)), and writes the K copies of
//                            swb_params the steps run with: state pointers = the scratch, actions = step k's block, outputs =
//                            step k's [N * M] slice, no frame, no overrides.
//   swb_rollout_kernel       one wave per virtual environment, built like swb_ms_state_kernel (the wide task scratch and one
//                            centred path in LDS, whatever the handle: tuned and many-sprite handles alike).  It runs the three
//                            shared pieces of the state phase K times, iteration k with copy k -- so a candidate auto-resets
//                            from pool_base + (episode mod pool_len) exactly as the live environment would.
// Why the copies are made by the fork launch and not in the wave: the pieces index swb_params::tasks with a loop variable, and a
// copy on the wave's stack that is indexed so stays in scratch memory (measured: 1936 bytes per lane).  Written by an earlier
// launch, copy k is read the way kernel arguments are -- constant address space, scalar loads.
// Between two iterations the wave re-reads what its own lanes stored (lane 0: step_count, reset_next, entry, nspr, episode;
// lanes < S: positions): wave_sync() orders them, and all of those words are read with plain global loads (THE RULE above:
// nothing written in this launch goes through as_const; pool_base / pool_len and the copies do, the fork launch wrote them).
// --------------------------------------------------------------------------------------------
#ifndef SWB_WIDE_TU
struct swb_rollout_args {
  int32_t M, K;
  // ---- scratch: the state of the N * M virtual environments
  double *x, *y;                 // [N * M][S]
  int32_t *nspr, *entry, *step_count, *episode, *pool_base, *pool_len;   // [N * M]
  uint8_t* reset_next;           // [N * M]
  swb_params* steps;             // [K] the virtual environments' view of the engine at step k
  // ---- io of the call (swb_rollout_outputs; any output may be NULL)
  const void* actions;           // [K][N * M][4] f64 / f32, or [K][N * M][2] i32
  double* reward;                // [K][N * M]
  float* discount;
  uint8_t *step_type, *success;
  uint8_t* error;                // [N * M] sticky
  double *out_x, *out_y;         // [N * M][S]
  int32_t* out_n;                // [N * M]
};
static_assert(sizeof(swb_params) + sizeof(swb_rollout_args) <= 4096, "kernel arguments of the rollout kernels");

__global__ void __launch_bounds__(256)
swb_rollout_fork_kernel(const swb_params p, const swb_rollout_args a) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);         // (N * M * S < 2^31: swb_rollout checks)
  if (idx < a.K) {
    const size_t o = (size_t)idx * p.N * a.M;
    const size_t action_bytes = p.action_space == SWB_ACTION_EMBODIED ? 2 * sizeof(int32_t) : (p.action_is_f32 ? 4 * sizeof(float) : 4 * sizeof(double));
    swb_params q = p;
    q.x = a.x; q.y = a.y; q.nspr = a.nspr; q.entry = a.entry; q.step_count = a.step_count; q.episode = a.episode;
    q.reset_next = a.reset_next; q.pool_base = a.pool_base; q.pool_len = a.pool_len;
    q.obs = nullptr; q.error = nullptr; q.render_only = 0; q.active = nullptr;
    q.actions = reinterpret_cast<const unsigned char*>(a.actions) + o * action_bytes;
    q.reward = a.reward ? a.reward + o : nullptr;
    q.discount = a.discount ? a.discount + o : nullptr;
    q.step_type = a.step_type ? a.step_type + o : nullptr;
    q.success = a.success ? a.success + o : nullptr;
    a.steps[idx] = q;
  }
  if (idx >= p.N * a.M * p.S) return;
  const int v = idx / p.S, s = idx - v * p.S, n = v / a.M;
  a.x[idx] = p.x[(size_t)n * p.S + s];
  a.y[idx] = p.y[(size_t)n * p.S + s];
  if (s == 0) {
    a.nspr[v] = p.nspr[n]; a.entry[v] = p.entry[n]; a.step_count[v] = p.step_count[n]; a.episode[v] = p.episode[n];
    a.reset_next[v] = p.reset_next[n];
    a.pool_base[v] = p.pool_base[n]; a.pool_len[v] = p.pool_len[n];
  }
}

// swb_reset_envs: environment n resets at its next active step where mask[n] != 0; nothing else is touched.
__global__ void __launch_bounds__(256)
swb_reset_envs_kernel(uint8_t* reset_next, const uint8_t* mask, int N) {
  const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (n < N && mask[n] != 0) reset_next[n] = 1;
}

// The per-environment state arrays a launch reads and writes (swb_params "live state", and the pool range beside it): the live
// ones, the scratch of a rollout's virtual environments, or a staging block of picked candidates (swb_rollout_frames).
struct swb_state_view {
  double *x, *y;                 // [n][S]
  int32_t *nspr, *entry, *step_count, *episode, *pool_base, *pool_len;   // [n]
  uint8_t* reset_next;           // [n]
};

// swb_rollout_frames with picked candidates: one thread per (environment, sprite) copies the state of virtual environment
// n * M + clamp(cand[n], 0, M - 1) from the rollout's scratch `src` into block `dst` of N environments, which one render launch
// then draws.  Plain vector loads and stores, like the fork kernel.
__global__ void __launch_bounds__(256)
swb_rollout_pick_kernel(const swb_state_view src, const swb_state_view dst, const int32_t* cand, int N, int S, int M) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);         // (N * S <= N * M * S < 2^31: swb_rollout checked)
  if (idx >= N * S) return;
  const int n = idx / S, s = idx - n * S;
  const size_t v = (size_t)n * M + (size_t)min(max(cand[n], 0), M - 1);
  dst.x[idx] = src.x[v * S + s];
  dst.y[idx] = src.y[v * S + s];
  if (s == 0) {
    dst.nspr[n] = src.nspr[v]; dst.entry[n] = src.entry[v]; dst.step_count[n] = src.step_count[v]; dst.episode[n] = src.episode[v];
    dst.reset_next[n] = src.reset_next[v];
    dst.pool_base[n] = src.pool_base[v]; dst.pool_len[n] = src.pool_len[v];
  }
}

// Snapshots (swb_save_state, swb_load_state): the nine arrays of a state move between the handle and a caller's block of C slots.
// Both kernels are the pick kernel's copy with the index the other way round or the same way, and without its clamp: plain
// vector loads and stores, one thread per (slot, sprite) or (environment, sprite), the words of an environment by the thread of
// sprite 0.  Source and destination are different allocations (the handle's, the caller's), so nothing a launch writes is read
// in it (THE RULE); no cross-lane operation.
//   swb_state_save_kernel   slot c takes element index[c] (NULL: c) of `src`, the live state or a rollout's scratch of n_src
//                           elements; an index outside [0, n_src) leaves the slot as it is.
__global__ void __launch_bounds__(256)
swb_state_save_kernel(const swb_state_view src, const swb_state_view dst, const int32_t* index, int C, int S, int n_src) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);         // (C * S < 2^31: swb_save_state checks)
  if (idx >= C * S) return;
  const int c = idx / S, s = idx - c * S;
  const int e = index ? index[c] : c;
  if (e < 0 || e >= n_src) return;
  dst.x[idx] = src.x[(size_t)e * S + s];
  dst.y[idx] = src.y[(size_t)e * S + s];
  if (s == 0) {
    dst.nspr[c] = src.nspr[e]; dst.entry[c] = src.entry[e]; dst.step_count[c] = src.step_count[e]; dst.episode[c] = src.episode[e];
    dst.reset_next[c] = src.reset_next[e];
    dst.pool_base[c] = src.pool_base[e]; dst.pool_len[c] = src.pool_len[e];
  }
}

//   swb_state_load_kernel   live environment n takes slot slot[n] (NULL: n) of the snapshot `src`; -1 leaves it exactly as it
//                           is, any other value outside [0, C) too and is counted in *rejected (may be NULL).  The thread of
//                           sprite 0 also clears the environment's SWB_RHDR_STAMP where the handle has run-list headers (rhdr;
//                           NULL: none): its next cover wave then finds no stamp of any epoch, builds its lists and resets
//                           SWB_RHDR_FRAME, whatever the sprites it was given do in that launch.  Environments that are not
//                           loaded keep stamp, lists and cached frame.
__global__ void __launch_bounds__(256)
swb_state_load_kernel(const swb_state_view src, const swb_state_view dst, const int32_t* slot, int C, int N, int S, uint32_t* rhdr,
                      int32_t* rejected) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);         // (N * S < 2^31, as in swb_factors_kernel)
  if (idx >= N * S) return;
  const int n = idx / S, s = idx - n * S;
  const int c = slot ? slot[n] : n;
  if (c < 0 || c >= C) {
    if (s == 0 && c != -1 && rejected) atomicAdd(rejected, 1);
    return;
  }
  dst.x[idx] = src.x[(size_t)c * S + s];
  dst.y[idx] = src.y[(size_t)c * S + s];
  if (s == 0) {
    dst.nspr[n] = src.nspr[c]; dst.entry[n] = src.entry[c]; dst.step_count[n] = src.step_count[c]; dst.episode[n] = src.episode[c];
    dst.reset_next[n] = src.reset_next[c];
    dst.pool_base[n] = src.pool_base[c]; dst.pool_len[n] = src.pool_len[c];
    if (rhdr) rhdr[(size_t)n * SWB_RHDR_DWORDS + SWB_RHDR_STAMP] = 0u;
  }
}

// swb_rollout_trajectory: where swb_rollout_kernel<true> keeps the state every step leaves.  `traj` is laid out like the scratch
// with [K][N * M] in front of every array -- slot k of virtual environment v is element k * N * M + v --, so that the view
// advanced by k * N * M + c * N is a valid swb_state_view of N environments for a render launch.  pool_base / pool_len do not
// change during a rollout and are not replicated (traj.pool_base / traj.pool_len are not used: a render view takes the scratch's).
// out_x, out_y [K][N * M][S] and out_n [K][N * M] are the caller's swb_rollout_step_outputs, any of them NULL.
struct swb_rollout_keep {
  swb_state_view traj;
  double *out_x, *out_y;
  int32_t* out_n;
};
static_assert(sizeof(swb_params) + sizeof(swb_rollout_args) + sizeof(swb_rollout_keep) <= 4096, "kernel arguments of the rollout kernels");

// swb_rollout_step_frames with picked candidates: one thread per (step, environment, sprite) copies slot k0 + kk of virtual
// environment n * M + clamp(cand[n], 0, M - 1) from the trajectory block `src` into environment kk * N + n of block `dst` (nk * N
// environments, drawn in nk render launches of N); pool_base / pool_len come from the rollout's scratch `pool`.  Plain vector
// loads and stores, like swb_rollout_pick_kernel.
__global__ void __launch_bounds__(256)
swb_rollout_pick_steps_kernel(const swb_state_view src, const swb_state_view pool, const swb_state_view dst, const int32_t* cand, int N,
                              int S, int M, int k0, int nk) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);         // (nk * N * S <= K * N * M * S < 2^31: swb_rollout_trajectory checked)
  if (idx >= nk * N * S) return;
  const int e = idx / S, s = idx - e * S, kk = e / N, n = e - kk * N;
  const size_t v = (size_t)n * M + (size_t)min(max(cand[n], 0), M - 1);
  const size_t slot = (size_t)(k0 + kk) * N * M + v;
  dst.x[idx] = src.x[slot * S + s];
  dst.y[idx] = src.y[slot * S + s];
  if (s == 0) {
    dst.nspr[e] = src.nspr[slot]; dst.entry[e] = src.entry[slot]; dst.step_count[e] = src.step_count[slot];
    dst.episode[e] = src.episode[slot]; dst.reset_next[e] = src.reset_next[slot];
    dst.pool_base[e] = pool.pool_base[v]; dst.pool_len[e] = pool.pool_len[v];
  }
}

// Register budget: the state phase is latency-bound (dependent loads, LDS round trips), so more resident waves win although the
// kernel then spills: measured at N = 1024, M = 64, K = 16 (goal_s5 / embodied_s12), 4 waves per SIMD (105 VGPRs, no spills)
// 1.430 / 1.338 ms, 5 waves (94 VGPRs, 2 spilled) 1.259 / 1.179 ms, 6 waves (80 VGPRs, 16 spilled) 1.194 / 1.121 ms.
// (profiles/r09_rollouts.md, section 2)
#ifndef SWB_ROLLOUT_WAVES_PER_SIMD
#define SWB_ROLLOUT_WAVES_PER_SIMD 6
#endif
// KEEP (swb_rollout_trajectory): every step the wave also writes its virtual environment's state into slot k of `keep`, from
// the registers the step's own stores were made from -- es.px / es.py are the words lanes < S hold in x, y (act_and_move stores
// them, a FIRST step's load_env_state does), es.n, es.en and the step count are what lane 0 stored or left, the episode number is
// counted along (a FIRST step adds one) -- so nothing just written is read back, and the stores are issued BEFORE the wave_sync()
// that ends the iteration: they drain together with the step's own (re-reading behind the wave_sync() was measured 24 to 35 %
// slower than swb_rollout, profiles/r14_rollout_trajectory.md).  reset_next after step k is whether step k + 1 is FIRST, which
// only the next iteration's load_env_state knows: slot k's byte is written then, the last slot's after the loop from memory
// (a plain load behind the wave_sync(): THE RULE).
#ifndef SWB_ROLLOUT_KEEP_WAVES_PER_SIMD
#define SWB_ROLLOUT_KEEP_WAVES_PER_SIMD 6
#endif
// SAMPLE (swb_rollout_sampled): the wave draws every step's action itself, after load_env_state, from the sprites the step acts
// on -- rollout_drawer<true>, written beside swb_sample_actions_kernel in swb_sampler.hip.inc (the Philox stream is defined
// there) -- and the drawn action replaces es.act / es.acti in registers.  Builds of their own, with a register budget of their
// own: measured at N = 1024, M = 64, K = 16 (goal_s5 / embodied_s12), uniform draws, 4 waves per SIMD 1.594 / 1.438 ms, 5 waves
// (96 VGPRs, 10 spilled) 1.490 / 1.299 ms, 6 waves (80 VGPRs, 26 spilled) 1.397 / 1.231 ms; clicks on sprites 1.884 / 1.960,
// 1.716 / 1.735, 1.584 / 1.614 ms.  (profiles/r15_rollout_random.md, section 2)
#ifndef SWB_ROLLOUT_SAMPLED_WAVES_PER_SIMD
#define SWB_ROLLOUT_SAMPLED_WAVES_PER_SIMD 6
#endif
struct swb_rollout_sample_args {
  int32_t mode;                // enum swb_action_sampling
  uint64_t seed, first_env;
  void* actions;               // [K][N * M][4] f64 / f32 or [K][N * M][2] i32: what was drawn
  int32_t *sprite, *tries;     // [K][N * M], ON_SPRITE only, may be NULL
};
static_assert(sizeof(swb_rollout_args) + sizeof(swb_rollout_keep) + sizeof(swb_rollout_sample_args) + 8 <= 4096,
              "kernel arguments of swb_rollout_kernel");
template <bool SAMPLE> struct rollout_drawer {};        // (the actions are the caller's: nothing to draw)
template <> struct rollout_drawer<true>;                // swb_sampler.hip.inc
template <bool KEEP, bool SAMPLE>
__global__ void __launch_bounds__(SWB_WAVE, SAMPLE ? SWB_ROLLOUT_SAMPLED_WAVES_PER_SIMD
                                                   : (KEEP ? SWB_ROLLOUT_KEEP_WAVES_PER_SIMD : SWB_ROLLOUT_WAVES_PER_SIMD))
swb_rollout_kernel(const swb_rollout_args a, int S, const swb_rollout_keep keep, const swb_rollout_sample_args sa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int l = lane_id();
  const int v = blockIdx.x;
  swb_ms_lds* M = reinterpret_cast<swb_ms_lds*>(smem);
  task_scratch_t<SWB_MAX_SPRITES>* tscratch = &M->ts;
  double2* cpath = M->path;
  uint32_t err = 0;
  int ep = 0;                                           // KEEP: the episode number the virtual environment is in
  if constexpr (KEEP) ep = a.episode[v];                // (written by the fork launch)
  rollout_drawer<SAMPLE> drawer;
  if constexpr (SAMPLE) drawer.start(sa, v / a.M, v % a.M);
  for (int k = 0; k < a.K; ++k) {
    const swb_params& q = *(const swb_params*)as_const(a.steps + k);
    env_state es = load_env_state<false, false>(q, v, tscratch);
    if constexpr (SAMPLE) drawer.draw(sa, q, k, es, cpath);
    // sprite.py:113-115 contains_point of sprite s2 (wave-uniform), as in swb_ms_state_kernel: its centred path into LDS,
    // lanes = vertices, then the even-odd test
    auto hit = [&](int s2, double tx, double ty) __attribute__((always_inline)) {
      const int nv = __builtin_amdgcn_readlane(es.nv_l, s2), so = __builtin_amdgcn_readlane(es.so_l, s2);
      const double sc = readlane_d(es.scale_l, s2), ca = readlane_d(es.ca_l, s2), sa = readlane_d(es.sa_l, s2);
      wave_sync();                                      // (the previous sprite's test has read the path)
      if (l < nv) {
        double cx, cy;
        centered_vertex(q, so, l, sc, ca, sa, cx, cy);
        cpath[l] = make_double2(cx, cy);
      }
      wave_sync();
      return contains_point_wave(cpath, nv, tx, ty);
    };
    const step_cost sc = act_and_move(q, v, es, hit);
    err |= finish_step<false, false>(q, v, es, sc, tscratch);       // (forked parameter blocks: no task cache, compiled out)
    if constexpr (KEEP) {
      const size_t slot = (size_t)k * gridDim.x + v;    // (one workgroup per virtual environment: gridDim.x = N * M)
      ep += es.first ? 1 : 0;
      if (l < S) {
        keep.traj.x[slot * S + l] = es.px;
        keep.traj.y[slot * S + l] = es.py;
        if (keep.out_x) keep.out_x[slot * S + l] = es.px;
        if (keep.out_y) keep.out_y[slot * S + l] = es.py;
      }
      if (l == 0) {
        keep.traj.nspr[slot] = es.n; keep.traj.entry[slot] = es.en; keep.traj.step_count[slot] = sc.step_count;
        keep.traj.episode[slot] = ep;
        if (k > 0) keep.traj.reset_next[slot - gridDim.x] = es.first ? 1 : 0;
        if (keep.out_n) keep.out_n[slot] = es.n;
      }
    }
    wave_sync();                                        // the next iteration reads what this one stored (state words, LDS scratch)
  }
  if constexpr (KEEP) {
    if (l == 0) keep.traj.reset_next[(size_t)(a.K - 1) * gridDim.x + v] = a.reset_next[v];
  }
  if (l < S) {
    if (a.out_x) a.out_x[(size_t)v * S + l] = a.x[(size_t)v * S + l];
    if (a.out_y) a.out_y[(size_t)v * S + l] = a.y[(size_t)v * S + l];
  }
  if (l == 0) {
    if (a.out_n) a.out_n[v] = a.nspr[v];
    if (a.error && err) a.error[v] |= (uint8_t)err;     // sticky: the caller clears
  }
}

// GUIDED (swb_rollout_guided): the wave draws every step's action from the caller's plan distribution of (step, environment) --
// a categorical over sprite indices, a uniform point inside the chosen sprite where it is now, a bell-shaped motion around a
// mean -- rollout_guided_drawer, beside rollout_drawer<true> in swb_sampler.hip.inc.  Kernels of their own, not a run-time mode
// of the SAMPLE builds: those sit at their register limit, and a drawer handed to swb_rollout_kernel as a template argument
// renames its four builds, while a body shared through an inlined function was compiled to other code for them (2 more spilled
// VGPRs in the plain build).  So the step loop below is swb_rollout_kernel's, line for line, with the other drawer; a change to
// one is a change to both.  Register budget: profiles/r24_rollout_guided.md.
#ifndef SWB_ROLLOUT_GUIDED_WAVES_PER_SIMD
#define SWB_ROLLOUT_GUIDED_WAVES_PER_SIMD 6
#endif
struct swb_rollout_guided_args {
  uint64_t seed, first_env;
  void* actions;               // [K][N * M][4] f64 / f32 or [K][N * M][2] i32: what was drawn
  int32_t *sprite, *tries;     // [K][N * M], may be NULL (tries: NULL for Embodied)
  const double* cdf;           // [K][N][W] running sums of the choice weights, or NULL: uniform choice
  const double *mean, *std;    // [K][N][2] of the motion; NULL for Embodied
  int32_t W, N;                // the plan's width; the environments of the handle (the plan's row of (k, n) is k * N + n)
};
static_assert(sizeof(swb_rollout_args) + sizeof(swb_rollout_keep) + sizeof(swb_rollout_guided_args) + 8 <= 4096,
              "kernel arguments of swb_rollout_guided_kernel");
struct rollout_guided_drawer;                           // swb_sampler.hip.inc
template <bool KEEP, class DRAWER = rollout_guided_drawer>
__global__ void __launch_bounds__(SWB_WAVE, SWB_ROLLOUT_GUIDED_WAVES_PER_SIMD)
swb_rollout_guided_kernel(const swb_rollout_args a, int S, const swb_rollout_keep keep, const swb_rollout_guided_args ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int l = lane_id();
  const int v = blockIdx.x;
  swb_ms_lds* M = reinterpret_cast<swb_ms_lds*>(smem);
  task_scratch_t<SWB_MAX_SPRITES>* tscratch = &M->ts;
  double2* cpath = M->path;
  uint32_t err = 0;
  int ep = 0;                                           // KEEP: the episode number the virtual environment is in
  if constexpr (KEEP) ep = a.episode[v];                // (written by the fork launch)
  DRAWER drawer;
  drawer.start(ga, v / a.M, v % a.M);
  for (int k = 0; k < a.K; ++k) {
    const swb_params& q = *(const swb_params*)as_const(a.steps + k);
    env_state es = load_env_state<false, false>(q, v, tscratch);
    drawer.draw(ga, q, k, es, cpath);
    auto hit = [&](int s2, double tx, double ty) __attribute__((always_inline)) {
      const int nv = __builtin_amdgcn_readlane(es.nv_l, s2), so = __builtin_amdgcn_readlane(es.so_l, s2);
      const double sc = readlane_d(es.scale_l, s2), ca = readlane_d(es.ca_l, s2), sa = readlane_d(es.sa_l, s2);
      wave_sync();                                      // (the previous sprite's test has read the path)
      if (l < nv) {
        double cx, cy;
        centered_vertex(q, so, l, sc, ca, sa, cx, cy);
        cpath[l] = make_double2(cx, cy);
      }
      wave_sync();
      return contains_point_wave(cpath, nv, tx, ty);
    };
    const step_cost sc = act_and_move(q, v, es, hit);
    err |= finish_step<false, false>(q, v, es, sc, tscratch);       // (forked parameter blocks: no task cache, compiled out)
    if constexpr (KEEP) {
      const size_t slot = (size_t)k * gridDim.x + v;    // (one workgroup per virtual environment: gridDim.x = N * M)
      ep += es.first ? 1 : 0;
      if (l < S) {
        keep.traj.x[slot * S + l] = es.px;
        keep.traj.y[slot * S + l] = es.py;
        if (keep.out_x) keep.out_x[slot * S + l] = es.px;
        if (keep.out_y) keep.out_y[slot * S + l] = es.py;
      }
      if (l == 0) {
        keep.traj.nspr[slot] = es.n; keep.traj.entry[slot] = es.en; keep.traj.step_count[slot] = sc.step_count;
        keep.traj.episode[slot] = ep;
        if (k > 0) keep.traj.reset_next[slot - gridDim.x] = es.first ? 1 : 0;
        if (keep.out_n) keep.out_n[slot] = es.n;
      }
    }
    wave_sync();                                        // the next iteration reads what this one stored (state words, LDS scratch)
  }
  if constexpr (KEEP) {
    if (l == 0) keep.traj.reset_next[(size_t)(a.K - 1) * gridDim.x + v] = a.reset_next[v];
  }
  if (l < S) {
    if (a.out_x) a.out_x[(size_t)v * S + l] = a.x[(size_t)v * S + l];
    if (a.out_y) a.out_y[(size_t)v * S + l] = a.y[(size_t)v * S + l];
  }
  if (l == 0) {
    if (a.out_n) a.out_n[v] = a.nspr[v];
    if (a.error && err) a.error[v] |= (uint8_t)err;     // sticky: the caller clears
  }
}
#endif  // SWB_WIDE_TU
#endif  // SWB_SETS_PASS
