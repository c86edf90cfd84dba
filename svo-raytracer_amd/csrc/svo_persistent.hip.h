// svo_persistent.hip.h -- pipeline 1: persistent waves, whole paths, lane refill.
//
// Each wave keeps 64 traversals in flight.  A lane owns one PATH at a time: its primary
// ray, then -- regenerated in place from the hit -- its bounce / shadow ray(s); when the
// path ends the lane stores the pixel and takes the next pixel of its XCD's screen band.
// Finished lanes are handled in rounds: once at most 9/16 of the lanes that were traversing
// at the start of a burst of trips are still traversing (the default; svo_set_tuning), the
// stopped lanes shade together (ballot), regenerate or retire, and the
// freed lanes are refilled with one atomic per wave (ballot + prefix count).  Compared
// with one-thread-per-pixel (pipeline 0 = the reference's decomposition) no lane waits for
// the slowest ray of its tile; compared with stage-per-kernel wavefront tracing
// (pipeline 2) the bounce ray starts where its primary just warmed the caches, no path
// state travels through HBM and the frame has one tail instead of one per stage.
//
// Work distribution: the frame is cut into 8 strips of whole tile rows, one per XCD (each XCD
// has its own 4 MiB L2; neighbouring tiles walk the same subtrees), and a strip is walked column
// by column so that the pixels an XCD has in flight form a compact block.  A wave reads its XCD
// id from the hardware register and draws from that band's counter, then steals from the
// other bands.  Consecutive launches walk the columns in opposite directions (a frame starts
// where the previous one is finishing).  Placement is only a locality hint: any wave may render
// any pixel.
#pragma once
#include "svo_fused.hip.h"
#include "svo_grow.h"
#include "svo_persist_plan.h"
#include "svo_trav.h"
#include "svo_travloop.h"
#include "svo_travloop2.h"

#include <algorithm>
#include <cstdlib>

namespace svo {

// One 128-byte line per band counter.  With the 8 counters in one line every refill atomic of every CU
// serialised on it and -- vmcnt being in-order on gfx950 -- stalled the record load behind it: in-kernel
// stamps (SVO_STAMPS build) showed the load wait growing from 420 to 2000 cycles per iteration as rounds
// became more frequent; with separate lines it stays below 500.
constexpr int kHeadStride = 32;
#ifdef SVO_STAMPS
constexpr int kHeadWords = 8 * kHeadStride + 32 + 64 + 64 + 16;  // + diagnostics words + the histograms of lanes traversing / popping per trip
                                                                   // + 8 x u64: cycles of a round by part
#else
constexpr int kHeadWords = 8 * kHeadStride + 32;  // + diagnostics words
#endif

struct PersistArgs {
  const uint8_t *pool;
  Frame f;
  uint32_t *color;
  float *depth;
  uint4 *hits;
  float *facc;       // spp > 1: colour sums (3 planes of npix)
  size_t npix;
  uint32_t *heads;   // 8 band counters (pixel slots drawn so far; with a ray list: its entries drawn, and in word kFillWord of the band's
                     // line the entries written)
  int tiles_per_band;  // unread since the row-major band walk went: kept, because without it hipcc allocates the kernels' registers differently
  int rows_per_band;   // tile rows per XCD band
  int reverse;         // walk the columns right to left (every other launch)
  int sample;        // sample index of this launch (one launch per sample), 0 when the launch carries all samples
  int fold;          // samples per pixel carried by this launch (see persist_plan); 1 = one launch per sample
  int group;         // fold > 1: tiles per group of a band's walk (sample by sample inside a group)
  int thresh_num;    // a round starts once active lanes <= thresh_num/16 of those active at its start
  // reciprocals (udiv_magic) of a band's tile rows and of its tile slots per frame, for a full band and for the last one
  uint32_t mg_rows[2], mg_tpf[2];
  // interior-descriptor table (svo_derive.hip.h); only read by the kDerived kernels
  const uint2 *desc;
  const uint2 *aux;
  uint32_t desc_count;
  // per-frame cameras and frame numbers of a batch (svo_ring_submit_cams), f.batch entries; only read by the kCams kernels
  const FrameVar *fvar;
  // path records of the spare-ray kernel (variants/svo_persist2.hip.h): kRecWaveWords words per persistent wave of the launch
  uint32_t *prec;
  int spare;   // 1 = launch the spare-ray kernel
  // row / column tables of the launch's frames (rc_table_kernel; only read by the kTab kernels): per frame rc_stride floats =
  // W column records {ra, u} then H row records {a.x, a.y, a.z, rb, b.x, b.y, b.z, 0}
  const float *rc;
  uint32_t rc_stride;
  const float4 *ntab;   // unit normals by 16-bit code (svo_trav2.h), or null
  // 1 = a band slot is a pixel with all the frames of the batch (persist_span_kernel): chosen once, in persist_plan
  int span;
  uint4 *prim;          // ... and the primary-hit records of its lanes, kSpanWords words per persistent lane of the launch
  // the context's primary-hit cache (persist_kept_kernel): three planes of kept_n records, a pixel's at its frame-0 output index
  // less kept_origin (the output index of the launch's first pixel row)
  uint4 *kept;          // null: the launch does not use the cache
  uint32_t kept_n, kept_origin;
  int kept_fill;        // 1 = this launch writes the cache (persist_kept_kernel<true>), 0 = it reads it
};

__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 7u;
}

// the live shader's pixel (one sample, no accumulation): the marker in the corner, then rgba8.  Alpha is 255: no such word is 0.
__device__ __forceinline__ uint32_t persist_rgba8(const Frame &f, int px, int py, V3 col) {
  if (px < 10 && py < 10) col = f.dword0 == 0u ? mk(1.f, 0.f, 0.f) : mk(1.f, 1.f, 1.f);
  return unorm8(col.x) | (unorm8(col.y) << 8) | (unorm8(col.z) << 16) | 0xff000000u;
}

// `sk`: sample index (bits 0..15) and frame of the batch (bits 16..23) of this path when the launch carries all samples of
// its pixels (a.fold > 1), else 0
__device__ __forceinline__ void persist_emit(const PersistArgs &a, uint32_t pix, uint32_t sk, int px, int py, V3 col, float depth) {
  const uint32_t smp = sk & 0xffffu;
  // (a kernel that stores nothing was a compile-time experiment: the ceiling of any staging scheme, profiles/round4_experiments.txt)
  if (a.f.spp <= 1 && !a.f.progressive) {   // the live shader's case: straight to rgba8
    a.color[pix] = persist_rgba8(a.f, px, py, col);
  } else if (a.fold > 1) {
    // every sample in a slot of its own, [frame][tile][sample][channel][pixel of the tile]: the 64 values of a tile's
    // sample and channel share two cache lines, and the kernel that adds the samples up in order reads them coalesced
    const int ry = py - a.f.y0;
    const uint32_t ty = a.f.row_step == 1 ? (uint32_t)(ry >> 3) : (uint32_t)(ry >> 3) / (uint32_t)a.f.row_step;
    const uint32_t tile = ty * (uint32_t)a.f.tiles_x + (uint32_t)(px >> 3), l = (uint32_t)(((ry & 7) << 3) | (px & 7));
    float *p = a.facc + (((size_t)(sk >> 16) * (size_t)a.f.ntiles + tile) * (size_t)a.fold + smp) * 192 + l;
    p[0] = col.x; p[64] = col.y; p[128] = col.z;
  } else {   // several samples and / or cross-frame accumulation: float sums, finished by persist_resolve_kernel
    float *fx = a.facc + pix, *fy = a.facc + a.npix + pix, *fz = a.facc + 2 * a.npix + pix;
    if (a.sample == 0) { *fx = 0.0f + col.x; *fy = 0.0f + col.y; *fz = 0.0f + col.z; }
    else { *fx = *fx + col.x; *fy = *fy + col.y; *fz = *fz + col.z; }
  }
  // the depth image is the first sample's; of a progressive sequence (every "sample" a frame of its own) the last frame's
  if (a.sample == 0 && smp == (a.f.seq > 1 ? (uint32_t)(a.fold - 1) : 0u)) a.depth[pix] = depth;
}

// SVO_ASM_LOOP=1 (default): the trips run in trav_loop() / trav_loop2() (gfx950 assembly);
// SVO_ASM_LOOP=0: hipcc's translation of trav_step() / trav_step2() -- same results, kept for A/B runs and as the
// readable form.
#ifndef SVO_ASM_LOOP
#define SVO_ASM_LOOP 1
#endif

// How a cast reads the octree.  ByteWalk: the reference's records, one fetched per iteration (svo_trav.h).
// DescWalk: the interior-descriptor table derived from them (svo_derive.hip.h, svo_trav2.h); the pool itself is only
// read for the record of the node a cast ends on.
struct ByteWalk {
#if SVO_ASM_LOOP
  typedef TravRegs State;
#else
  typedef Trav State;
#endif
  typedef WaveStack Stack;
  BufPool pool;
  uint64_t root;
  __device__ __forceinline__ void setup(const PersistArgs &a) {
    pool = make_bufpool(a.pool, a.f.pool_len);
    root = load_record(pool, 0u);
  }
  __device__ __forceinline__ int init(State &t, V3 o, V3 d, bool cone, float t_start = 0.0f) const {
#if SVO_ASM_LOOP
    return trav_init_regs(root, t, o, d, cone, t_start);
#else
    return trav_init(root, t, o, d, cone, t_start);
#endif
  }
  __device__ __forceinline__ void fresh_stack(Stack &, uint32_t) const {}   // the record walk keeps a "pushed" mask per ray
  __device__ __forceinline__ Cast result(const State &t, int status) const {
#if SVO_ASM_LOOP
    return trav_result_regs(pool, t, status);
#else
    return trav_result(t, status);
#endif
  }
  // trips until at most `threshold` of the lanes in `act` are still traversing
  __device__ __forceinline__ void run(Stack &stk, uint32_t lane, State &t, int &status, unsigned long long act, int threshold,
                                      unsigned long long cone_lanes, uint32_t *mix) const {
#if SVO_ASM_LOOP
    trav_loop(pool, stk, lane, t, status, act, threshold, cone_lanes, mix);
#else
    (void)act; (void)cone_lanes; (void)mix;
    for (;;) {
#ifdef SVO_STAMPS
      unsigned long long st_load = 0;
      if (status == ST_ACTIVE) status = trav_step(pool, stk, lane, t, st_load);
#else
      if (status == ST_ACTIVE) status = trav_step(pool, stk, lane, t);
#endif
      if (__builtin_popcountll(__ballot(status == ST_ACTIVE)) <= threshold) break;
    }
#endif
  }
};

struct DescWalk {
#if SVO_ASM_LOOP
  typedef TravRegs2 State;
#else
  typedef Trav2 State;
#endif
  typedef WaveStack2 Stack;
  BufPool pool;
  DescTab tab;
  uint2 rootd;
  __device__ __forceinline__ void setup(const PersistArgs &a) {
    pool = make_bufpool(a.pool, a.f.pool_len);
    tab = make_desctab(a.desc, a.aux, a.desc_count, a.ntab);
    const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(tab.rsrc, (int)kDescRoot, 0, 0);
    rootd = make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)r.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y));
  }
  __device__ __forceinline__ int init(State &t, V3 o, V3 d, bool cone, float t_start = 0.0f) const {
#if SVO_ASM_LOOP
    return trav_init_regs2(rootd, t, o, d, cone, t_start);
#else
    return trav_init2(rootd, t, o, d, cone, t_start);
#endif
  }
  // a new ray starts on a zeroed stack column, like the reference's zero-initialised stack[] (svotrace.comp:227): a pop to a
  // level the ray never pushed then reads {descriptor 0, t_max 0} by itself, and the loop keeps no "pushed" mask
  __device__ __forceinline__ void fresh_stack(Stack &stk, uint32_t lane) const {
#if SVO_ASM_LOOP
    // (always in the assembly build: trav_loop2's POP reads its entry without a pushed-levels mask.  Round 3's closing
    // commit lost the define that guarded these stores and shipped a kernel without them; tests/test_kernel_isa.py checks
    // the shipped one.  What the stores cost was priced once with a compile-time switch that built a WRONG kernel:
    // profiles/round4_experiments.txt, "noclear".)
#pragma unroll
    for (int lv = 0; lv < kStackLevels; ++lv) stk.pm[lane + 64u * (uint32_t)lv] = make_uint2(0u, 0u);
#else
    (void)stk; (void)lane;
#endif
  }
  __device__ __forceinline__ Cast result(const State &t, int status) const {
#if SVO_ASM_LOOP
    return trav_result_regs2(pool, tab, t, status);
#else
    return trav_result2(pool, tab, t, status);
#endif
  }
  // where a stopped cast stopped, for a caller that reads nothing else of the result: no load (result() fetches the node's record)
  __device__ __forceinline__ float stop_t(const State &t) const { return t.t_min; }
  __device__ __forceinline__ void run(Stack &stk, uint32_t lane, State &t, int &status, unsigned long long act, int threshold,
                                      unsigned long long cone_lanes, uint32_t *mix) const {
#if SVO_ASM_LOOP
    trav_loop2(tab, stk, lane, t, status, act, threshold, cone_lanes, mix);
#else
    (void)act; (void)cone_lanes; (void)mix;
    for (;;) {
      if (status == ST_ACTIVE) status = trav_step2(tab, stk, lane, t);
      if (__builtin_popcountll(__ballot(status == ST_ACTIVE)) <= threshold) break;
    }
#endif
  }
};

#ifndef SVO_DRAIN_NUM
#define SVO_DRAIN_NUM 12
#endif
#ifndef SVO_PERSIST_WAVES_PER_SIMD
#define SVO_PERSIST_WAVES_PER_SIMD 5
#endif
#ifndef SVO_DERIVED_WAVES_PER_SIMD
#define SVO_DERIVED_WAVES_PER_SIMD 6
#endif
template <class Walk> struct WalkWaves { static constexpr int value = SVO_PERSIST_WAVES_PER_SIMD; };
template <> struct WalkWaves<DescWalk> { static constexpr int value = SVO_DERIVED_WAVES_PER_SIMD; };

// kCams: the frames of the batch carry their own camera and frameNumber (a.fvar) -- a kernel of its own, so that the
// static-camera kernel keeps the camera in SGPRs from its kernel arguments
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
// kTab: the row and column parts of a new pixel's pure functions come from tables made once per launch (rc_table_kernel) instead
// of being evaluated in every round for a third of the lanes -- of the primary direction (svotrace.comp:662-675) the two
// divisions of the pixel centre and the six mixes along the left and right edge vectors (functions of the row) and the
// horizontal fraction (of the column); of the pixel's random number (:26-29, :486) the two inner sin / fract chains (one a
// function of the column and frameNumber, one of the row and frameNumber).  What stays in the round: three mixes, the
// normalisation, the outer chain -- the same operations on the same values, so the same bits.
// kSpan (persist_span_kernel; mode 0, one camera, one sample per pixel, f.batch > 1, f.bounces >= 2, no beam): a band slot is a
// PIXEL, not a (frame, pixel) pair.  The frames of such a batch differ in frameNumber only, and frameNumber first enters a path in
// scatter(), behind the primary cast (the pixel's random number): the primary ray of a pixel is the same ray in every frame of the
// batch.  The lane casts it once, keeps what the shading of a primary hit reads (direction, voxel position, normal, value, t:
// kSpanWords words) in a record of its own in global memory (a.prim: written once per pixel, read once per further frame;
// registers would cost the kernel its sixth wave per SIMD), and runs frame 0's path, frame 1's, ... from that hit, each with its
// own random number -- the same operations on the same values in the same order as the (frame, pixel) slots, so the same bytes.
// (kSpanWords, svo_persist_plan.h: three uint4 per persistent lane, [wave][3][lane])
constexpr uint32_t kSpanSun = 1u << 16;   // in a kSpan lane's `seg`: a miss of the segment under way adds the sun's light
constexpr uint32_t kKeptMiss = 1u;        // in the last word of a cached record's third plane: the primary ray left the octree
// kKept (persist_kept_kernel<true>, the fill): the kSpan kernel with a pixel's record in the context's cache (a.kept) instead of
// its lane's own, and a record for the primaries that leave the octree too.
template <int kMode, class Walk, bool kCams, bool kTab, bool kSpan, bool kKept = false>
__device__ __forceinline__ void persist_body(const PersistArgs &a, typename Walk::Stack &stk) {
  static_assert(!kSpan || (kMode == 0 && !kCams), "a batch shares its primary ray only in mode 0 with one camera");
  static_assert(!kKept || kSpan, "the cache keeps the primary hits of a kSpan launch");
  const uint32_t lane = threadIdx.x;
  const Frame &f = a.f;
  Walk walk;
  walk.setup(a);
  const V3 cam_o = mk(f.cam[0], f.cam[1], f.cam[2]);
  const V3 sun2 = normalize3(mk(0.5f, 0.5f, 0.5f));

  typename Walk::State t;
  int status = ST_IDLE;
  uint32_t pix = 0, seg = 0;   // seg: path segment in the low byte; a.fold > 1: sample index in bits 8..23, frame of the batch above
                               // (kSpan: the frame the lane's pixel has reached, in the same place)
  int px = 0, py = 0;  // path state that outlives a cast
  V3 d = mk(0.f, 0.f, 0.f), mask = mk(1.f, 1.f, 1.f), accum = mk(0.f, 0.f, 0.f), normal = mk(0.f, 0.f, 0.f);
  float r = 0.0f, depth = 0.0f;
  uint32_t value = 0;

  uint32_t band = xcc_id();
  int bands_left = 8;

#ifdef SVO_STAMPS
  unsigned long long st_round = 0, st_trav = 0, st_nround = 0, st_ntrip = 0, st_shade = 0, st_load = 0, st_t0 = __builtin_readcyclecounter();
  const unsigned long long st_begin = __builtin_amdgcn_s_memrealtime();   // 100 MHz, one clock for the whole device
  unsigned long long st_dry = 0;
  uint32_t st_mix[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // trips / lanes, by section (trav_loop); [8], [9]: per-lane histogram words (trav_loop2)
  // a round by part (round 6): the cast's result (hit-record fetch + decode), the shading arithmetic, the pixel store, the refill
  // (counter draw + the new pixels' primary direction / random number), the ray set-up (three IEEE divisions + the stack column)
  unsigned long long st_part[5] = {0, 0, 0, 0, 0}, st_lanes_shaded = 0, st_lanes_refilled = 0, st_lanes_init = 0;
#endif
  for (;;) {
    // ---------------- finished lanes: shade, then regenerate the next ray in place or retire
    // A lane leaves this block with a pixel to store (emit) and / or a new ray to set up (ninit); the store and the
    // set-up run once per round, behind the refill, for all the lanes that need them together -- not once per branch
    // (three copies of the store, two of the set-up with its three IEEE divisions, each for a handful of lanes).
    bool emit = false, ninit = false, icone = false;
    V3 ecol = mk(0.f, 0.f, 0.f), io = mk(0.f, 0.f, 0.f);
    float edepth = 0.0f, its = 0.0f;
#ifdef SVO_STAMPS
    unsigned long long st_r1 = 0, st_r2 = 0;
    st_lanes_shaded += (unsigned long long)__builtin_popcountll(__ballot(status >= ST_HIT));
#endif
    if (status >= ST_HIT) {
      Cast c = walk.result(t, status);
#ifdef SVO_STAMPS
      asm volatile("" ::"v"(c.t), "v"(c.pointer), "v"(c.normal.x), "v"(c.voxel_pos.x), "v"(c.value) : "memory");   // the record is here
      st_r1 = __builtin_readcyclecounter();
#endif
      status = ST_IDLE;
      const uint32_t segn = seg & 0xffu, smp = seg >> 8;   // smp: sample | frame of the batch << 16
      if (segn == 0u && (smp & 0xffffu) == 0u && f.write_hits && a.sample == 0) {
        uint4 h;
        h.x = c.hit ? c.pointer : 0u;
        h.y = c.hit ? ((c.raw & 0xffffu) | ((c.value & 0xffu) << 16) | ((c.level & 0xffu) << 24)) : 0u;
        h.z = c.iter;
        h.w = c.hit ? __float_as_uint(c.t) : 0u;
        if (kMode == 4) h = make_uint4(0u, 0u, 0u, 0u);   // trace() casts nothing in modes >= 4 (svotrace.comp:643-646)
        a.hits[pix] = h;
        if (kSpan)   // the one primary cast is every frame's: the same record into every frame's plane
          for (int k = 1; k < f.batch; k++) a.hits[pix + (uint32_t)k * f.frame_stride] = h;
      }
      emit = true;
      if constexpr (kSpan) {
        // One shading per stopped lane and round, whatever the lane does next.  A cast that ends its frame's path -- a bounce that
        // left the octree, or the hit of the last segment -- needs no scatter() of its own here: what a miss adds was decided when
        // the ray was set up (kSpanSun, below), and a last hit emits the sums as they stand.  So the lane emits, takes its
        // pixel's next frame (the primary hit from its record, that frame's random number) and shades THAT in the same pass as the
        // lanes whose primary or inner segment just hit.  (persist_plan: f.bounces >= 2, so a shaded hit always goes on.)
        // (the address is formed here, in the round: hoisted in front of the kernel's loop it is two registers spilled for good)
        uint32_t rl = lane;
        asm volatile("" : "+v"(rl));
        // (kKept: the pixel's record in the cache; `pix` is frame (seg >> 24)'s output index here)
        uint4 *const rec = kKept ? a.kept + (pix - (seg >> 24) * f.frame_stride - a.kept_origin)
                                 : a.prim + (size_t)blockIdx.x * (64u * kSpanWords / 4u) + rl;   // [3][64] uint4 per wave
        const uint32_t rs = kKept ? a.kept_n : 64u;   // records between two planes
        const V3 sun = normalize3(mk(1.0f, 1.0f, 1.0f));
        bool shade = true;
        if (segn == 0u) {
          if (c.hit) {   // the pixel's primary hit, for all its frames
            rec[0] = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), __float_as_uint(c.t));
            rec[rs] = make_uint4(__float_as_uint(c.voxel_pos.x), __float_as_uint(c.voxel_pos.y), __float_as_uint(c.voxel_pos.z), c.value);
            rec[2u * rs] = make_uint4(__float_as_uint(c.normal.x), __float_as_uint(c.normal.y), __float_as_uint(c.normal.z), 0u);
            emit = false;
          } else {
            if (kKept) {   // a miss is kept too: the direction its sky is a function of, and the flag (kKeptMiss)
              rec[0] = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), 0u);
              rec[2u * rs] = make_uint4(0u, 0u, 0u, kKeptMiss);
            }
            const V3 s = sky_colour(d);
            ecol = mk(0.0f + s.x, 0.0f + s.y, 0.0f + s.z);
            shade = false;
          }
        } else if (!c.hit || (int)segn + 1 >= f.bounces) {   // frame (seg >> 24)'s path ends
          if (c.hit) {
            accum = mk(accum.x + mask.x * 0.0f, accum.y + mask.y * 0.0f, accum.z + mask.z * 0.0f);
            edepth = c.t;
          } else {
            if ((seg & kSpanSun) != 0u) accum = mk(accum.x + mask.x * 7.0f, accum.y + mask.y * 7.0f, accum.z + mask.z * 7.0f);
            accum = mk(accum.x + mask.x * 1.0f, accum.y + mask.y * 1.0f, accum.z + mask.z * 1.0f);
          }
          // (stored here, not behind the block with the other lanes' pixels: the colour would stay live across the shading below,
          // four registers the kernel does not have)
          persist_emit(a, pix, 0u, px, py, accum, edepth);
          emit = false;
          const uint32_t fi = (seg >> 24) + 1u;
          shade = fi < (uint32_t)f.batch;
          if (shade) {   // the pixel's next frame: a refilled lane's path state, the primary hit as it was
            const uint4 r0 = rec[0], r1 = rec[rs], r2 = rec[2u * rs];
            d = mk(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
            c.t = __uint_as_float(r0.w);
            c.voxel_pos = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
            c.value = r1.w;
            c.normal = mk(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
            seg = fi << 24;
            pix += f.frame_stride;
            mask = mk(1.f, 1.f, 1.f);
            accum = mk(0.f, 0.f, 0.f);
            if (kTab) {
              const float *fr = a.rc + (size_t)fi * a.rc_stride;
              const float colx = fr[2 * px], roww = fr[((2 * f.width + 3) & ~3) + 8 * py + 3];
              r = rand_of_dot(((float)px + colx) * 12.9898f + ((float)py + roww) * 78.233f);
            } else {
              r = pixel_rand((float)px, (float)py, (float)(f.frame_number + (int)fi + a.sample));
            }
          }
        } else {
          emit = false;   // an inner segment's hit
        }
        if (shade) {   // a hit the path goes on from: the same operations as below
          normal = c.normal; value = c.value;
          const V3 vpos = c.voxel_pos;
          const bool mirror = ((f.mirror_mask >> (value & 31u)) & 1u) != 0u;
          const V3 nd = scatter(d, normal, r, mirror);
          const V3 mc = material_colour(value, mk(vpos.x - 1.0f, vpos.y - 1.0f, vpos.z - 1.0f));
          depth = c.t;
          accum = mk(accum.x + mask.x * 0.0f, accum.y + mask.y * 0.0f, accum.z + mask.z * 0.0f);
          mask = mk(mask.x * mc.x, mask.y * mc.y, mask.z * mc.z);
          const float k = dot3(nd, normal);
          mask = mk(mask.x * k, mask.y * k, mask.z * k);
          d = nd;
          seg++;
          ninit = true; icone = true; io = vpos;
          status = ST_ACTIVE;
          // kSpanSun: should the new ray leave the octree, the path ends with scatter(d, normal, r) of exactly these values (a
          // miss changes neither normal nor value) against the sun: one bit, taken now, while the lane shades anyway.  Every
          // shaded hit pays for this second scatter(), the hit of an inner segment too, whether or not its next ray misses:
          // per path that is the scatter() the (frame, pixel) kernel runs when the path ends, moved here.  The bit equals that
          // kernel's only because both inlined copies of scatter() are the same IEEE operations (-ffp-contract=off, no
          // fast-math); tests/test_gpu_batch_primary.py holds the bytes against it and against the oracle.
          const V3 nd2 = scatter(d, normal, r, mirror);
          seg = acos_pinned(dot3(nd2, sun)) < 0.4f ? (seg | kSpanSun) : (seg & ~kSpanSun);
        }
      } else if (kMode == 0) {
        if (segn == 0u && !c.hit) {
          const V3 s = sky_colour(d);
          ecol = mk(0.0f + s.x, 0.0f + s.y, 0.0f + s.z);
        } else {
          V3 vpos = mk(0.f, 0.f, 0.f);
          if (c.hit) { normal = c.normal; value = c.value; vpos = c.voxel_pos; }
          const V3 nd = scatter(d, normal, r, ((f.mirror_mask >> (value & 31u)) & 1u) != 0u);
          if (c.hit) {
            const V3 mc = material_colour(value, mk(vpos.x - 1.0f, vpos.y - 1.0f, vpos.z - 1.0f));
            depth = c.t;
            accum = mk(accum.x + mask.x * 0.0f, accum.y + mask.y * 0.0f, accum.z + mask.z * 0.0f);
            mask = mk(mask.x * mc.x, mask.y * mc.y, mask.z * mc.z);
            const float k = dot3(nd, normal);
            mask = mk(mask.x * k, mask.y * k, mask.z * k);
            if ((int)segn + 1 >= f.bounces) {
              ecol = accum; edepth = depth;
            } else {
              d = nd;
              seg++;
              emit = false; ninit = true; icone = true; io = vpos;
              status = ST_ACTIVE;   // not idle: keeps its pixel (the set-up behind the refill gives the real status)
            }
          } else {
            const V3 sun = normalize3(mk(1.0f, 1.0f, 1.0f));
            const float diff = acos_pinned(dot3(nd, sun));
            if (diff < 0.4f) accum = mk(accum.x + mask.x * 7.0f, accum.y + mask.y * 7.0f, accum.z + mask.z * 7.0f);
            accum = mk(accum.x + mask.x * 1.0f, accum.y + mask.y * 1.0f, accum.z + mask.z * 1.0f);
            ecol = accum;
          }
        }
      } else if (kMode == 1) {
        if (c.hit) { const float g = 0.005f * (float)c.iter; ecol = mk(g, g, g); }
        else if (c.capped) ecol = mk(0.3f, 0.3f, 0.6f);
        else { const float g = 0.01f * (float)c.iter; ecol = mk(g, g, g); }
        edepth = c.hit ? c.t : 0.0f;
      } else if (kMode == 2) {
        if (segn == 0u) {
          if (c.hit) {
            V3 mc = material_colour(c.value, kMode2OtherMaterial);
            const float k = (c.level >= 10u ? dot3(c.normal, sun2) : dot3(mk(0.f, 1.0f, 0.f), sun2)) * 0.1f;
            mc = mk(mc.x + k, mc.y + k, mc.z + k);
            const float dist = c.t + 0.0f;
            const float lg = exp2_pinned(dist * (-0.5f * 2.0f * 1.44269504f));
            const float lb = exp2_pinned(dist * (-0.5f * 4.0f * 1.44269504f));
            const float lr = exp2_pinned(dist * (-0.5f * 1.0f * 1.44269504f));
            mc.x = lr * mc.x + (1.0f - lr) * 1.0f;
            mc.y = lg * mc.y + (1.0f - lg) * 1.0f;
            mc.z = lb * mc.z + (1.0f - lb) * 1.0f;
            mask = mc;
            depth = c.t;
            seg = (seg & ~0xffu) | 1u;
            d = sun2;   // (the primary direction is not needed any more)
            emit = false; ninit = true; icone = false; io = c.voxel_pos;
            status = ST_ACTIVE;
          } else {
            ecol = sky_colour(d);
          }
        } else {
          V3 mc = mask;
          if (c.hit && c.t > c.scale_exp2 * 1.73205080757f) {
            mc = mk(mc.x - 0.2f, mc.y - 0.2f, mc.z - 0.2f);
          } else if (c.iter > 260u) {
            const float pen = (0.05f * (float)c.iter) / 100.0f;
            mc = mk(mc.x - pen, mc.y - pen, mc.z - pen);
          }
          ecol = mc; edepth = depth;
        }
      } else if (kMode == 3) {
        if (c.hit) { ecol = mk(c.normal.x * 0.5f + 0.5f, c.normal.y * 0.5f + 0.5f, c.normal.z * 0.5f + 0.5f); edepth = c.t; }
      }
    }
#ifdef SVO_STAMPS
    asm volatile("" ::"v"(ecol.x), "v"(ecol.y), "v"(ecol.z), "v"(edepth), "v"(io.x), "v"(d.x) : "memory");
    st_r2 = __builtin_readcyclecounter();
    {
      // st_r1 is per lane (taken under the branch): the wave's figure = the largest (the lanes that took the branch share one clock read)
      unsigned long long m = st_r1;
      for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(m, o, 64); m = x > m ? x : m; }
      if (m != 0) { st_part[0] += m - st_t0; st_part[1] += st_r2 - m; }
    }
#endif
    if (emit) {
      if (kSpan) {
        // (only primary misses come here: the same sky in every frame of the batch)
        for (int k = 0; k < f.batch; k++) persist_emit(a, pix + (uint32_t)k * f.frame_stride, 0u, px, py, ecol, edepth);
      } else {
        persist_emit(a, pix, seg >> 8, px, py, ecol, edepth);
      }
    }

#ifdef SVO_STAMPS
    { const unsigned long long now = __builtin_readcyclecounter(); st_shade += now - st_t0; st_part[2] += now - st_r2; st_r2 = now; }
#endif
    // ---------------- refill idle lanes: ballot + prefix count, one atomic per wave
    // (a wave whose band is used up tries the next band in its next round; trying it in the same round was a compile-time
    // experiment: 1-4 % slower -- tools/history/r03_ab_drain.sh, profiles/round3_experiments.txt)
    uint32_t cam_frame = 0u; int cam_sample = 0; bool cam_fresh = false;   // kCams only
    while (bands_left > 0) {
      const unsigned long long idle = __ballot(status == ST_IDLE);
      if (idle == 0ull) break;
      {
        const uint32_t n = (uint32_t)__builtin_popcountll(idle);
        const int leader = __builtin_ctzll(idle);
        // a band = a strip of whole tile rows, walked column by column: the pixels in flight on an XCD form a compact
        // block of the screen (strip height x a few dozen tile columns) instead of two or three full-width tile rows
        const int first_row = (int)band * a.rows_per_band;
        int band_rows = f.tiles_y - first_row;
        band_rows = band_rows < 0 ? 0 : (band_rows > a.rows_per_band ? a.rows_per_band : band_rows);
        const uint32_t band_frame = (uint32_t)(band_rows * f.tiles_x) * 64u;   // pixel slots of the band in one frame
        // ... and over the launch's frames x samples (kSpan: a slot is a pixel, with all its frames)
        const uint32_t band_total = kSpan ? band_frame : band_frame * (uint32_t)(f.batch * a.fold);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(a.heads + band * kHeadStride, n);
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);   // wave-uniform, and the compiler knows it
        const uint32_t slot =
            base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (status == ST_IDLE && slot < band_total) {
          const uint32_t l = slot & 63u;
          // frames of a batch follow one another inside the band: a wave that runs out of frame k goes on with k + 1
          // ; the samples of a pixel (a.fold > 1) follow one another tile by tile: tile 0 sample 0, 1, ..., tile 1 sample 0,
          // ... -- what is in flight at any time are a few tiles' samples, whose primary rays are the same and whose
          // slots in the sample buffer are neighbours
          // (the two divisions of every refill -- by the band's tile slots per frame and by its tile rows -- are
          // multiply-highs by reciprocals made on the host)
          const uint32_t per_frame = band_frame * (uint32_t)a.fold;
          const uint32_t tiles_pf = per_frame >> 6;   // tile slots of the band per frame
          const int full_band = band_rows == a.rows_per_band ? 0 : 1;
          const uint32_t fi = !kSpan && f.batch > 1 ? udiv_by(slot >> 6, tiles_pf, a.mg_tpf[full_band]) : 0u;
          const uint32_t q = (slot - fi * per_frame) >> 6;
          uint32_t si = 0u;
          int j = (int)q;
          if (a.fold > 1) {   // groups of a.group tiles: sample 0 of the group's tiles, sample 1 of them, ...
            const uint32_t tiles = band_frame >> 6, g = q / ((uint32_t)a.group * (uint32_t)a.fold);
            const uint32_t first = g * (uint32_t)a.group;
            const uint32_t gsize = tiles - first < (uint32_t)a.group ? tiles - first : (uint32_t)a.group;
            const uint32_t r = q - first * (uint32_t)a.fold;
            si = r / gsize;
            j = (int)(first + r % gsize);
          }
          int tile_x = (int)udiv_by((uint32_t)j, (uint32_t)band_rows, a.mg_rows[full_band]);
          const int tile_y = first_row + (j - tile_x * band_rows);
          if (a.reverse) tile_x = f.tiles_x - 1 - tile_x;   // serpentine: this frame ends where the next one starts
          px = tile_x * 8 + (int)(l & 7u);
          py = frame_gy(f, tile_y, (int)(l >> 3));
          if (px < f.width && py < f.y1 && py < f.height) {
            pix = fi * f.frame_stride + (uint32_t)frame_oy(f, tile_y, (int)(l >> 3)) * (uint32_t)f.width + (uint32_t)px;
            if (kTab) {
              const float *fr = a.rc + (size_t)fi * a.rc_stride;
              const float2 col = *(const float2 *)(fr + 2 * px);
              const float *rowp = fr + ((2 * f.width + 3) & ~3) + 8 * py;   // (row records start on a 16-byte boundary)
              const float4 ra4 = *(const float4 *)rowp, rb4 = *(const float4 *)(rowp + 4);
              d = normalize3(mk(mix_g(ra4.x, rb4.x, col.y), mix_g(ra4.y, rb4.y, col.y), mix_g(ra4.z, rb4.z, col.y)));
              if (kMode == 0) r = rand_of_dot(((float)px + col.x) * 12.9898f + ((float)py + ra4.w) * 78.233f);
            } else if (!kCams) d = primary_direction(f, px, py);
            seg = a.fold > 1 ? (si << 8) | (fi << 24) : 0u;
            mask = mk(1.f, 1.f, 1.f);
            accum = mk(0.f, 0.f, 0.f);
            normal = mk(0.f, 0.f, 0.f);
            value = 0u;
            depth = 0.0f;
            if (kMode == 0 && !kCams && !kTab) r = pixel_rand((float)px, (float)py, (float)(f.frame_number + (int)fi + a.sample + (int)si));
            if (kCams) { cam_frame = fi; cam_sample = a.sample + (int)si; cam_fresh = true; }
            ninit = true; icone = false; io = cam_o; its = beam_start(f, px, py);
            status = ST_ACTIVE;   // taken (the set-up below gives the real status)
          }
        }
        if (kCams) {
          // the camera of every refilled lane's frame: the slots of one draw are consecutive, so nearly always all lanes
          // are in one frame -- one 64-byte scalar load per distinct frame, the lanes of that frame take their ray from it
          unsigned long long todo = __ballot(cam_fresh);
          while (todo != 0ull) {
            const uint32_t fu = (uint32_t)__builtin_amdgcn_readlane((int)cam_frame, __builtin_ctzll(todo));
            const FrameVar *vp = a.fvar + fu;
            u32x16 raw;   // = *vp: cam[0..14], frame_number
            asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(raw) : "s"(vp) : "memory");
            const bool mine = cam_fresh && cam_frame == fu;
            if (mine) {
              float cam[15];
#pragma unroll
              for (int i = 0; i < 15; i++) cam[i] = __uint_as_float(raw[i]);
              if (!kTab) d = primary_direction_cam(cam, f.width, f.height, px, py);
              io = mk(cam[0], cam[1], cam[2]);
              if (kMode == 0 && !kTab) r = pixel_rand((float)px, (float)py, (float)((int)raw[15] + cam_sample));
              cam_fresh = false;
            }
            todo &= ~__ballot(mine);
          }
        }
        if (base + n >= band_total) {  // this band is used up: move on (work stealing)
          band = (band + 1u) & 7u;
          bands_left--;
#ifdef SVO_STAMPS
          if (bands_left == 0) st_dry = __builtin_amdgcn_s_memrealtime();
#endif
        }
        break;
      }
    }
#ifdef SVO_STAMPS
    asm volatile("" ::"v"(d.x), "v"(r), "v"(pix) : "memory");
    { const unsigned long long now = __builtin_readcyclecounter(); st_part[3] += now - st_r2; st_r2 = now; }
    st_lanes_init += (unsigned long long)__builtin_popcountll(__ballot(ninit));
    st_lanes_refilled += (unsigned long long)__builtin_popcountll(__ballot(ninit && !icone && (seg & 0xffu) == 0u));
#endif
    // ---------------- set up the new rays: regenerated bounce / shadow rays and refilled primaries together
    if (ninit) {
      status = walk.init(t, io, d, icone, its);
      walk.fresh_stack(stk, lane);
      if (kMode == 4) status = ST_MISS;   // no cast: straight to the (black) pixel
    }
    if (__ballot(status != ST_IDLE) == 0ull) {
      if (bands_left > 0) continue;
      break;
    }

#ifdef SVO_STAMPS
    { const unsigned long long now = __builtin_readcyclecounter(); st_part[4] += now - st_r2; st_round += now - st_t0; st_t0 = now; st_nround++; }
#endif
    // ---------------- traverse until enough lanes have stopped to make a round worthwhile
    const int active0 = __builtin_popcountll(__ballot(status == ST_ACTIVE));
    // (a fixed "N lanes free" trigger was tried instead of the proportional one: 3 % slower at its best setting)
    // once every band is used up a round only serves the lanes that go on with another segment of their path: they should
    // not wait for the longest cast of the wave (SVO_DRAIN_NUM/16 of the active lanes may still be traversing; 0 = wait for all)
    const int drained = (active0 * SVO_DRAIN_NUM) / 16 < active0 - 1 ? (active0 * SVO_DRAIN_NUM) / 16 : (active0 > 0 ? active0 - 1 : 0);
    const int threshold = __builtin_amdgcn_readfirstlane(bands_left > 0 ? (active0 * a.thresh_num) / 16 : drained);
    {
      const unsigned long long act = __ballot(status == ST_ACTIVE);
      // cone rays: the secondary segments of a GI path (svotrace.comp:446: coneTrace = i != 0)
#ifdef SVO_STAMPS
      uint32_t *const mixp = st_mix;
#else
      uint32_t *const mixp = nullptr;
#endif
      walk.run(stk, lane, t, status, act, __builtin_amdgcn_readfirstlane(threshold),
               kMode == 0 ? __ballot((seg & 0xffu) != 0u) : 0ull, mixp);
    }
#ifdef SVO_STAMPS
    { const unsigned long long now = __builtin_readcyclecounter(); st_trav += now - st_t0; st_t0 = now; }
#endif
  }
#ifdef SVO_STAMPS
  if (lane == 0u) {
    unsigned long long *dbg = (unsigned long long *)(a.heads + 8 * kHeadStride);  // spare words behind the 8 band counters
    const unsigned long long st_end = __builtin_amdgcn_s_memrealtime();
    atomicMax(dbg + 6, ~st_begin); atomicMax(dbg + 7, ~st_dry); atomicMax(dbg + 8, st_dry); atomicMax(dbg + 9, st_end);
    atomicAdd(dbg + 10, st_end - st_begin); atomicAdd(dbg + 11, st_dry - st_begin);
    for (int i = 0; i < 8; i += 2)   // dbg[12..15]: lanes << 32 | trips, for the whole trip / descend / advance / pop
      atomicAdd(dbg + 12 + i / 2, ((unsigned long long)st_mix[i + 1] << 32) + st_mix[i]);

  }
  atomicAdd(a.heads + 8 * kHeadStride + 32 + lane, st_mix[8]);
  atomicAdd(a.heads + 8 * kHeadStride + 32 + 64 + lane, st_mix[9]);
  if (lane == 0u) {
    unsigned long long *parts = (unsigned long long *)(a.heads + 8 * kHeadStride + 32 + 64 + 64);
    for (int i = 0; i < 5; i++) atomicAdd(parts + i, st_part[i]);
    atomicAdd(parts + 5, st_lanes_shaded); atomicAdd(parts + 6, st_lanes_init); atomicAdd(parts + 7, st_lanes_refilled);
  }
  if (lane == 0u) {
    unsigned long long *dbg = (unsigned long long *)(a.heads + 8 * kHeadStride);
    atomicAdd(dbg + 0, st_round); atomicAdd(dbg + 1, st_trav); atomicAdd(dbg + 2, st_nround); atomicAdd(dbg + 3, st_ntrip); atomicAdd(dbg + 4, st_shade); atomicAdd(dbg + 5, st_load);
  }
#endif
}

template <int kMode, class Walk, bool kCams = false, bool kTab = false>
__global__ __launch_bounds__(64, WalkWaves<Walk>::value) void persist_kernel(const PersistArgs a) {
  __shared__ typename Walk::Stack stk;
  persist_body<kMode, Walk, kCams, kTab, false>(a, stk);
}

// a static-camera batch of mode 0 on the descriptor walk: one primary cast per pixel for all the frames of the batch (kSpan)
template <bool kTab>
__global__ __launch_bounds__(64, WalkWaves<DescWalk>::value) void persist_span_kernel(const PersistArgs a) {
  __shared__ DescWalk::Stack stk;
  persist_body<0, DescWalk, false, kTab, true>(a, stk);
}

// The shading of a hit a mode-0 path goes on from, as persist_body's kSpan branch states it -- ONE text for the two places that
// run it from a kept primary hit: persist_reuse_body in its rounds and bounce_rays_kernel ahead of the walk.  (persist_body's kSpan
// branch keeps its own statement: called from there, persist_span_kernel<true> spills 16 bytes instead of 8.)  The same operations
// in the same order (-ffp-contract=off, no fast-math), so the same bits wherever it is inlined.  Two functions because the reuse
// kernel runs them a traversal apart: shade_hit() when the hit is known -- the new direction, the sums, and `sun_lit`: should the new
// ray leave the octree, the path ends with scatter() of exactly these values against the sun (kSpanSun) -- and path_end() when the
// cast has said whether the path's last ray hit.
__device__ __forceinline__ V3 shade_hit(const Frame &f, V3 d, V3 hpos, V3 hnormal, uint32_t hvalue, float r, V3 &mask, V3 &accum, bool &sun_lit) {
  const V3 sun = normalize3(mk(1.0f, 1.0f, 1.0f));
  const bool mirror = ((f.mirror_mask >> (hvalue & 31u)) & 1u) != 0u;
  const V3 nd = scatter(d, hnormal, r, mirror);
  const V3 mc = material_colour(hvalue, mk(hpos.x - 1.0f, hpos.y - 1.0f, hpos.z - 1.0f));
  accum = mk(accum.x + mask.x * 0.0f, accum.y + mask.y * 0.0f, accum.z + mask.z * 0.0f);
  mask = mk(mask.x * mc.x, mask.y * mc.y, mask.z * mc.z);
  const float k = dot3(nd, hnormal);
  mask = mk(mask.x * k, mask.y * k, mask.z * k);
  const V3 nd2 = scatter(nd, hnormal, r, mirror);   // kSpanSun: what a miss of the new ray will add
  sun_lit = acos_pinned(dot3(nd2, sun)) < 0.4f;
  return nd;
}
__device__ __forceinline__ V3 path_end(V3 accum, V3 mask, bool hit, bool sun_lit) {
  if (hit) {
    accum = mk(accum.x + mask.x * 0.0f, accum.y + mask.y * 0.0f, accum.z + mask.z * 0.0f);
  } else {
    if (sun_lit) accum = mk(accum.x + mask.x * 7.0f, accum.y + mask.y * 7.0f, accum.z + mask.z * 7.0f);
    accum = mk(accum.x + mask.x * 1.0f, accum.y + mask.y * 1.0f, accum.z + mask.z * 1.0f);
  }
  return accum;
}

// The reuse of the context's primary-hit cache (persist_kept_kernel<false>): the kSpan kernel of a launch whose primary hits an
// earlier launch of the same camera, pool and frame left in a.kept (the fill).  A refilled lane casts nothing: it loads its
// pixel's record and shades frame 0 from it exactly as the kSpan kernel shades frames 1.. from its lane's own -- the same
// operations on the same values in the same order, so the same bytes.  The round's order differs: the lanes whose frame ended
// emit first, then slots are drawn and records loaded (a miss emits its sky into every frame and its lane draws again in the same
// round, while the band has slots), and only then ONE shading pass runs for the lanes holding a primary hit from a record or
// an inner hit from the cast: no refilled lane sits out a traversal phase waiting for the next round's shading.
// Mode 0, the descriptor walk, the row / column tables, one slot per pixel.
__device__ __forceinline__ void persist_reuse_body(const PersistArgs &a, DescWalk::Stack &stk) {
  const uint32_t lane = threadIdx.x;
  const Frame &f = a.f;
  DescWalk walk;
  walk.setup(a);

  DescWalk::State t;
  int status = ST_IDLE;
  uint32_t pix = 0, seg = 0;   // seg: path segment in the low byte, kSpanSun, the frame the lane's pixel has reached in bits 24..
  int px = 0, py = 0;
  V3 d = mk(0.f, 0.f, 0.f), mask = mk(1.f, 1.f, 1.f), accum = mk(0.f, 0.f, 0.f);
  float r = 0.0f;

  uint32_t band = xcc_id();
  int bands_left = 8;

  for (;;) {
    // ---------------- finished lanes: a path that ended stores its pixel and goes on to the pixel's next frame; an inner hit waits
    // for the shading pass
    bool shade = false, load = false;
    V3 hpos = mk(0.f, 0.f, 0.f), hnormal = mk(0.f, 0.f, 0.f);
    uint32_t hvalue = 0u;
    if (status >= ST_HIT) {
      const Cast c = walk.result(t, status);
      const uint32_t segn = seg & 0xffu;   // (never 0: no lane of this kernel casts a primary ray)
      if (!c.hit || (int)segn + 1 >= f.bounces) {   // frame (seg >> 24)'s path ends
        accum = path_end(accum, mask, c.hit, (seg & kSpanSun) != 0u);
        persist_emit(a, pix, 0u, px, py, accum, c.hit ? c.t : 0.0f);
        const uint32_t fi = (seg >> 24) + 1u;
        if (fi < (uint32_t)f.batch) {   // keeps its pixel
          seg = fi << 24;
          pix += f.frame_stride;
          load = true;
          status = ST_ACTIVE;
        } else {
          status = ST_IDLE;
        }
      } else {
        hpos = c.voxel_pos; hnormal = c.normal; hvalue = c.value;
        shade = true;
        status = ST_ACTIVE;   // not idle: keeps its pixel (the set-up below gives the real status)
      }
    }

    // ---------------- idle lanes draw pixels (ballot + prefix count, one atomic per wave: persist_body's walk of the bands with a
    // pixel per slot), then every lane at the start of a frame loads its pixel's record
    for (;;) {
      bool again = false;   // the band still has slots behind this draw
      const unsigned long long idle = bands_left > 0 ? __ballot(status == ST_IDLE) : 0ull;
      if (idle != 0ull) {
        const uint32_t n = (uint32_t)__builtin_popcountll(idle);
        const int leader = __builtin_ctzll(idle);
        const int first_row = (int)band * a.rows_per_band;
        int band_rows = f.tiles_y - first_row;
        band_rows = band_rows < 0 ? 0 : (band_rows > a.rows_per_band ? a.rows_per_band : band_rows);
        const uint32_t band_total = (uint32_t)(band_rows * f.tiles_x) * 64u;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(a.heads + band * kHeadStride, n);
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        const uint32_t slot =
            base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (status == ST_IDLE && slot < band_total) {
          const uint32_t l = slot & 63u, q = slot >> 6;
          const int full_band = band_rows == a.rows_per_band ? 0 : 1;
          int tile_x = (int)udiv_by(q, (uint32_t)band_rows, a.mg_rows[full_band]);
          const int tile_y = first_row + ((int)q - tile_x * band_rows);
          if (a.reverse) tile_x = f.tiles_x - 1 - tile_x;
          px = tile_x * 8 + (int)(l & 7u);
          py = frame_gy(f, tile_y, (int)(l >> 3));
          if (px < f.width && py < f.y1 && py < f.height) {
            pix = (uint32_t)frame_oy(f, tile_y, (int)(l >> 3)) * (uint32_t)f.width + (uint32_t)px;
            seg = 0u;
            load = true;
            status = ST_ACTIVE;   // taken
          }
        }
        if (base + n >= band_total) {   // this band is used up: the next one in the next round (work stealing)
          band = (band + 1u) & 7u;
          bands_left--;
        } else {
          again = true;
        }
      }
      if (load) {
        const uint32_t fi = seg >> 24;
        const uint4 *const rec = a.kept + (pix - fi * f.frame_stride - a.kept_origin);
        const uint4 r0 = rec[0], r1 = rec[a.kept_n], r2 = rec[2u * a.kept_n];
        load = false;
        d = mk(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
        if (r2.w == kKeptMiss) {   // (of a new pixel only: a pixel with a frame behind it hit) the same sky in every frame
          const V3 s = sky_colour(d);
          const V3 ecol = mk(0.0f + s.x, 0.0f + s.y, 0.0f + s.z);
          for (int k = 0; k < f.batch; k++) persist_emit(a, pix + (uint32_t)k * f.frame_stride, 0u, px, py, ecol, 0.0f);
          status = ST_IDLE;
        } else {   // the primary hit as it was (its t is no input of the shading), and frame fi's random number
          hpos = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
          hvalue = r1.w;
          hnormal = mk(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
          mask = mk(1.f, 1.f, 1.f);
          accum = mk(0.f, 0.f, 0.f);
          const float *fr = a.rc + (size_t)fi * a.rc_stride;
          const float colx = fr[2 * px], roww = fr[((2 * f.width + 3) & ~3) + 8 * py + 3];
          r = rand_of_dot(((float)px + colx) * 12.9898f + ((float)py + roww) * 78.233f);
          shade = true;
        }
      }
      if (!again || __ballot(status == ST_IDLE) == 0ull) break;
    }

    // ---------------- one shading pass: a hit the path goes on from (persist_plan: f.bounces >= 2), persist_body's kSpan shading
    bool ninit = false;
    if (shade) {
      bool sun_lit;
      d = shade_hit(f, d, hpos, hnormal, hvalue, r, mask, accum, sun_lit);
      seg++;
      ninit = true;
      seg = sun_lit ? (seg | kSpanSun) : (seg & ~kSpanSun);
    }
    // ---------------- set up the new rays
    if (ninit) {
      status = walk.init(t, hpos, d, true, 0.0f);
      walk.fresh_stack(stk, lane);
    }
    if (__ballot(status != ST_IDLE) == 0ull) {
      if (bands_left > 0) continue;
      break;
    }
    // ---------------- traverse until enough lanes have stopped to make a round worthwhile (persist_body)
    const int active0 = __builtin_popcountll(__ballot(status == ST_ACTIVE));
    const int drained = (active0 * SVO_DRAIN_NUM) / 16 < active0 - 1 ? (active0 * SVO_DRAIN_NUM) / 16 : (active0 > 0 ? active0 - 1 : 0);
    const int threshold = __builtin_amdgcn_readfirstlane(bands_left > 0 ? (active0 * a.thresh_num) / 16 : drained);
    walk.run(stk, lane, t, status, __ballot(status == ST_ACTIVE), threshold, ~0ull, nullptr);
  }
}

// a static-camera batch of mode 0 whose primary hits stay in the context's cache from launch to launch (persist_kept_choose):
// kFill = the kSpan kernel writing the cache, !kFill = the kernel that reads it and casts no primary ray
template <bool kFill>
__global__ __launch_bounds__(64, WalkWaves<DescWalk>::value) void persist_kept_kernel(const PersistArgs a) {
  __shared__ DescWalk::Stack stk;
  if constexpr (kFill) persist_body<0, DescWalk, false, true, true, true>(a, stk);
  else persist_reuse_body(a, stk);
}

// ---------------- the dense pass of a launch that reads the cache and whose paths are primary + one bounce (PersistPlan::dense)
// With f.bounces == 2 a (pixel, frame)'s path is decided before its bounce ray is cast, but for two facts: did the ray hit, and at
// what t.  The direction, and the colour of either ending, are functions of the kept record, the row / column tables and the frame
// number; the hit's record is never read.  So the shading leaves the half-empty persistent waves: bounce_rays_kernel runs it at 64
// of 64 lanes for every (pixel, frame) and leaves a ray record; persist_cast_kernel only draws, loads, casts and stores.

// The ray records of a launch, [frame of the batch][pixel of the launch's rows, indexed like the cache]: kRayBytes each
struct RayArgs {
  uint4 *ray;       // {direction of the bounce ray, rgba8 should it miss}; w == 0 (no pixel's word: alpha is 255) = the pixel's PRIMARY
                    // ray left the octree: nothing to cast, bounce_rays_kernel has stored the sky
  uint32_t *hitc;   // rgba8 should it hit.  Not assumed black: a voxel with normal code 0 gives a NaN direction and NaN sums (quirk Q7)
  uint32_t n;       // records per frame
};

// One thread per (pixel of the launch's rows, frame of the batch); a workgroup = one wave = an 8 x 8 tile of one frame: the reads of
// the kept records and of the frame's tables coalesce.  The operations of persist_reuse_body on a refilled lane, in its order.
__global__ __launch_bounds__(64) void bounce_rays_kernel(const PersistArgs a, const RayArgs ra) {
  const Frame &f = a.f;
  const uint32_t l = threadIdx.x, fi = blockIdx.z;
  const int px = (int)(blockIdx.x * 8u + (l & 7u)), py = frame_gy(f, (int)blockIdx.y, (int)(l >> 3));
  if (px >= f.width || py >= f.y1 || py >= f.height) return;
  const uint32_t idx = (uint32_t)frame_oy(f, (int)blockIdx.y, (int)(l >> 3)) * (uint32_t)f.width + (uint32_t)px - a.kept_origin;
  const uint4 *const rec = a.kept + idx;
  const uint4 r0 = rec[0], r2 = rec[2u * a.kept_n];
  const V3 d = mk(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
  const size_t j = (size_t)fi * ra.n + idx;
  if (r2.w == kKeptMiss) {   // the same sky in every frame; persist_cast_kernel draws again when it meets the flag
    const V3 s = sky_colour(d);
    persist_emit(a, idx + a.kept_origin + fi * f.frame_stride, 0u, px, py, mk(0.0f + s.x, 0.0f + s.y, 0.0f + s.z), 0.0f);
    ra.ray[j] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint4 r1 = rec[a.kept_n];
  const V3 hpos = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
  const V3 hnormal = mk(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
  V3 mask = mk(1.f, 1.f, 1.f), accum = mk(0.f, 0.f, 0.f);
  const float *fr = a.rc + (size_t)fi * a.rc_stride;
  const float colx = fr[2 * px], roww = fr[((2 * f.width + 3) & ~3) + 8 * py + 3];
  const float r = rand_of_dot(((float)px + colx) * 12.9898f + ((float)py + roww) * 78.233f);
  bool sun_lit;
  const V3 nd = shade_hit(f, d, hpos, hnormal, r1.w, r, mask, accum, sun_lit);
  const uint32_t miss_c = persist_rgba8(f, px, py, path_end(accum, mask, false, sun_lit));
  ra.ray[j] = make_uint4(__float_as_uint(nd.x), __float_as_uint(nd.y), __float_as_uint(nd.z), miss_c);
  ra.hitc[j] = persist_rgba8(f, px, py, path_end(accum, mask, true, sun_lit));
}

// persist_reuse_body without its shading: the band walk and the draw (a slot per pixel), the trips, thresh_num and the drain rule are
// the same; a lane at the start of a frame loads that frame's ray record and the origin (the kept hit's position, plane 1 of the
// cache), and a stopped lane stores one of the record's two colour words.  Across the trips a lane keeps its walk state, its pixel,
// its frame and the two words.  A cast that hit the iteration cap counts as a miss, as Cast::hit == false does there.
__device__ __forceinline__ void persist_cast_body(const PersistArgs &a, const RayArgs &ra, DescWalk::Stack &stk) {
  const uint32_t lane = threadIdx.x;
  const Frame &f = a.f;
  DescWalk walk;
  walk.setup(a);

  DescWalk::State t;
  int status = ST_IDLE;
  uint32_t pix = 0, fi = 0, miss_c = 0, hit_c = 0;   // pix: frame fi's output index

  uint32_t band = xcc_id();
  int bands_left = 8;

  for (;;) {
    // ---------------- finished lanes store their pixel and go on to the pixel's next frame
    bool load = false;
    if (status >= ST_HIT) {
      const bool hit = status == ST_HIT;
      a.color[pix] = hit ? hit_c : miss_c;
      a.depth[pix] = hit ? walk.stop_t(t) : 0.0f;
      fi++;
      if (fi < (uint32_t)f.batch) {   // keeps its pixel
        pix += f.frame_stride;
        load = true;
        status = ST_ACTIVE;
      } else {
        status = ST_IDLE;
      }
    }

    // ---------------- idle lanes draw pixels (persist_reuse_body's draw), then every lane at the start of a frame loads its ray
    bool ninit = false;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    for (;;) {
      bool again = false;   // the band still has slots behind this draw
      const unsigned long long idle = bands_left > 0 ? __ballot(status == ST_IDLE) : 0ull;
      if (idle != 0ull) {
        const uint32_t n = (uint32_t)__builtin_popcountll(idle);
        const int leader = __builtin_ctzll(idle);
        const Band b = band_of(band, a.rows_per_band, f.tiles_x, f.tiles_y, 1, 1, true);   // a slot per pixel (svo_persist_plan.h)
        const uint32_t band_total = b.total;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(a.heads + band * kHeadStride, n);
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        const uint32_t slot =
            base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (status == ST_IDLE && slot < band_total) {
          const SlotPixel sp = slot_pixel(f, slot_tile(b, slot, a.rows_per_band, f.tiles_x, a.reverse, a.mg_rows, a.mg_tpf, 1, 1, 1, true));
          if (sp.inside) {
            pix = sp.pix;
            fi = 0u;
            load = true;
            status = ST_ACTIVE;   // taken
          }
        }
        if (base + n >= band_total) {   // this band is used up: the next one in the next round (work stealing)
          band = (band + 1u) & 7u;
          bands_left--;
        } else {
          again = true;
        }
      }
      if (load) {
        const uint32_t idx = pix - fi * f.frame_stride - a.kept_origin;
        const size_t j = (size_t)fi * ra.n + idx;
        const uint4 q = ra.ray[j];
        load = false;
        if (q.w == 0u) {   // (of a new pixel only) sky: stored already, the lane draws again while the band has slots
          status = ST_IDLE;
        } else {
          const uint4 r1 = a.kept[a.kept_n + idx];
          miss_c = q.w;
          hit_c = ra.hitc[j];
          o = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
          d = mk(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z));
          ninit = true;
        }
      }
      if (!again || __ballot(status == ST_IDLE) == 0ull) break;
    }
    // ---------------- set up the new rays
    if (ninit) {
      status = walk.init(t, o, d, true, 0.0f);
      walk.fresh_stack(stk, lane);
    }
    if (__ballot(status != ST_IDLE) == 0ull) {
      if (bands_left > 0) continue;
      break;
    }
    // ---------------- traverse until enough lanes have stopped to make a round worthwhile (persist_body)
    const int active0 = __builtin_popcountll(__ballot(status == ST_ACTIVE));
    const int drained = (active0 * SVO_DRAIN_NUM) / 16 < active0 - 1 ? (active0 * SVO_DRAIN_NUM) / 16 : (active0 > 0 ? active0 - 1 : 0);
    const int threshold = __builtin_amdgcn_readfirstlane(bands_left > 0 ? (active0 * a.thresh_num) / 16 : drained);
    walk.run(stk, lane, t, status, __ballot(status == ST_ACTIVE), threshold, ~0ull, nullptr);
  }
}

__global__ __launch_bounds__(64, WalkWaves<DescWalk>::value) void persist_cast_kernel(const PersistArgs a, const RayArgs ra) {
  __shared__ DescWalk::Stack stk;
  persist_cast_body(a, ra, stk);
}

// ---------------- the same pass with its ray records as a compact list (PersistPlan::list; ray_list_kernel + persist_runs_kernel)
// The ray list of a launch (svo_persist_plan.h, "the ray list"): kRayListBytes per record in two planes, cut into the 8 bands'
// regions (ray_region).  Only a (pixel, frame) that casts a ray has an entry: a pixel whose PRIMARY ray left the octree has its sky
// stored by ray_list_kernel and appears nowhere.  Per band two words of its line in a.heads, both zeroed by rc_table_kernel: word 0
// the draw cursor of persist_runs_kernel, word kFillWord the entries ray_list_kernel has written.
struct RayListArgs {
  uint4 *ray;   // {direction of the bounce ray, rgba8 should it miss}
  uint2 *tag;   // {rgba8 should it hit, cache index | frame << kRayIndexBits}.  The hit's colour is not assumed black: a voxel with
                // normal code 0 gives a NaN direction and NaN sums (quirk Q7)
};
constexpr uint32_t kFillWord = 1;

// bounce_rays_kernel's shading with a thread per PIXEL of the launch's rows: a workgroup = one wave = an 8 x 8 tile, which lies in one
// band; the thread loads the kept record once and shades the batch's frames one after the other -- the operations of
// persist_reuse_body on a refilled lane, in its order.  A tile's pixels that hit are the same in every frame, so the wave reserves
// room for all its entries with ONE atomic on the band's fill count (ballot + prefix count) and writes them frame by frame, each
// frame's as one contiguous run.  The list is compacted, not ordered: a key on the ray's direction was measured and dropped
// (profiles/ray_list.md).
__global__ __launch_bounds__(64) void ray_list_kernel(const PersistArgs a, const RayListArgs ra) {
  const Frame &f = a.f;
  const uint32_t l = threadIdx.x, nb = (uint32_t)f.batch;
  const int px = (int)(blockIdx.x * 8u + (l & 7u)), py = frame_gy(f, (int)blockIdx.y, (int)(l >> 3));
  const uint32_t band = blockIdx.y / (uint32_t)a.rows_per_band;
  const uint32_t idx = (uint32_t)frame_oy(f, (int)blockIdx.y, (int)(l >> 3)) * (uint32_t)f.width + (uint32_t)px - a.kept_origin;
  bool live = false;
  uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0, r2 = r0;
  if (px < f.width && py < f.y1 && py < f.height) {
    const uint4 *const rec = a.kept + idx;
    r0 = rec[0]; r2 = rec[2u * a.kept_n];
    if (r2.w == kKeptMiss) {   // the same sky in every frame, and no entry
      const V3 s = sky_colour(mk(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)));
      for (uint32_t fi = 0; fi < nb; fi++)
        persist_emit(a, idx + a.kept_origin + fi * f.frame_stride, 0u, px, py, mk(0.0f + s.x, 0.0f + s.y, 0.0f + s.z), 0.0f);
    } else {
      r1 = rec[a.kept_n];
      live = true;
    }
  }
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;
  const uint32_t n = (uint32_t)__builtin_popcountll(m);
  const int leader = __builtin_ctzll(m);
  uint32_t base = 0;
  if ((int)l == leader) base = atomicAdd(a.heads + band * kHeadStride + kFillWord, n * nb);
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
  if (!live) return;
  // (at most the band's pixels x frames are ever reserved: the entry stays inside the band's region)
  uint32_t e = ray_region(band, a.rows_per_band, f.tiles_y, f.width, f.batch).first + base +
               __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  const V3 d = mk(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
  const V3 hpos = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
  const V3 hnormal = mk(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
  for (uint32_t fi = 0; fi < nb; fi++, e += n) {
    V3 mask = mk(1.f, 1.f, 1.f), accum = mk(0.f, 0.f, 0.f);
    const float *fr = a.rc + (size_t)fi * a.rc_stride;
    const float colx = fr[2 * px], roww = fr[((2 * f.width + 3) & ~3) + 8 * py + 3];
    const float r = rand_of_dot(((float)px + colx) * 12.9898f + ((float)py + roww) * 78.233f);
    bool sun_lit;
    const V3 nd = shade_hit(f, d, hpos, hnormal, r1.w, r, mask, accum, sun_lit);
    ra.ray[e] = make_uint4(__float_as_uint(nd.x), __float_as_uint(nd.y), __float_as_uint(nd.z), persist_rgba8(f, px, py, path_end(accum, mask, false, sun_lit)));
    ra.tag[e] = make_uint2(persist_rgba8(f, px, py, path_end(accum, mask, true, sun_lit)), idx | (fi << kRayIndexBits));
  }
}

// persist_cast_body without its pixels: the trips, thresh_num and the drain rule are the same, and so is the walk of the 8 bands (the
// wave's XCD first, then stealing).  What a wave draws are ENTRIES of a band's ray list: it holds a wave-uniform run [cur, end) of
// them, reserved kChunk at a time with one atomic on the band's draw cursor (ray_run_reserve), and idle lanes take the run's next
// entries (ray_run_take), load their record and the origin (the kept hit's position, plane 1 of the cache) and cast.  A stopped lane
// stores one of the record's two colour words and is idle: no lane keeps a pixel from frame to frame, no entry is empty.  Across
// the trips a lane keeps its walk state, its output index and the two words.
__device__ __forceinline__ void persist_runs_body(const PersistArgs &a, const RayListArgs &ra, DescWalk::Stack &stk) {
  const uint32_t lane = threadIdx.x;
  const Frame &f = a.f;
  DescWalk walk;
  walk.setup(a);

  DescWalk::State t;
  int status = ST_IDLE;
  uint32_t pix = 0, miss_c = 0, hit_c = 0;

  uint32_t band = xcc_id();
  int bands_left = 8;
  RayRun run;   // wave-uniform
  run.cur = 0u; run.end = 0u; run.last = false;

  for (;;) {
    // ---------------- finished lanes store their pixel
    if (status >= ST_HIT) {
      const bool hit = status == ST_HIT;
      a.color[pix] = hit ? hit_c : miss_c;
      a.depth[pix] = hit ? walk.stop_t(t) : 0.0f;
      status = ST_IDLE;
    }

    // ---------------- idle lanes take the next entries of the wave's run; a run used up is followed by the band's next one in the same
    // round, a band used up by the next band in the next round (work stealing, as persist_body has it)
    bool ninit = false;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    while (bands_left > 0) {
      const unsigned long long idle = __ballot(status == ST_IDLE);
      if (idle == 0ull) break;
      if (run.cur == run.end) {
        if (run.last) {
          band = (band + 1u) & 7u;
          bands_left--;
          run.last = false;
          break;
        }
        const int leader = __builtin_ctzll(idle);
        uint32_t base = 0, filled = 0;
        if ((int)lane == leader) {
          base = atomicAdd(a.heads + band * kHeadStride, kChunk);
          filled = a.heads[band * kHeadStride + kFillWord];
        }
        run = ray_run_reserve((uint32_t)__builtin_amdgcn_readlane((int)base, leader), (uint32_t)__builtin_amdgcn_readlane((int)filled, leader));
        continue;
      }
      const uint32_t at = run.cur;
      const uint32_t n = ray_run_take(run, (uint32_t)__builtin_popcountll(idle));
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
      if (status == ST_IDLE && rank < n) {
        const uint32_t e = ray_region(band, a.rows_per_band, f.tiles_y, f.width, f.batch).first + at + rank;
        const uint4 q = ra.ray[e];
        const uint2 w = ra.tag[e];
        const uint32_t idx = w.y & kRayIndexMask;
        const uint4 r1 = a.kept[a.kept_n + idx];
        pix = idx + a.kept_origin + (w.y >> kRayIndexBits) * f.frame_stride;
        miss_c = q.w;
        hit_c = w.x;
        o = mk(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
        d = mk(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z));
        ninit = true;
        status = ST_ACTIVE;   // taken (the set-up below gives the real status)
      }
    }
    // ---------------- set up the new rays
    if (ninit) {
      status = walk.init(t, o, d, true, 0.0f);
      walk.fresh_stack(stk, lane);
    }
    if (__ballot(status != ST_IDLE) == 0ull) {
      if (bands_left > 0) continue;
      break;
    }
    // ---------------- traverse until enough lanes have stopped to make a round worthwhile (persist_body)
    const int active0 = __builtin_popcountll(__ballot(status == ST_ACTIVE));
    const int drained = (active0 * SVO_DRAIN_NUM) / 16 < active0 - 1 ? (active0 * SVO_DRAIN_NUM) / 16 : (active0 > 0 ? active0 - 1 : 0);
    const int threshold = __builtin_amdgcn_readfirstlane(bands_left > 0 ? (active0 * a.thresh_num) / 16 : drained);
    walk.run(stk, lane, t, status, __ballot(status == ST_ACTIVE), threshold, ~0ull, nullptr);
  }
}

__global__ __launch_bounds__(64, WalkWaves<DescWalk>::value) void persist_runs_kernel(const PersistArgs a, const RayListArgs ra) {
  __shared__ DescWalk::Stack stk;
  persist_runs_body(a, ra, stk);
}

// a.fold > 1: tiles per group of a band's walk.  1 / 8 / 64 / 512 / all: 4.47 / 4.49 / 4.47 / 4.41 / 4.20 Grays/s at 64
// samples per pixel (tools/history/r03_fold2.sh): a group's samples should be in flight together, not a whole band's
constexpr int kFoldGroup = 8;
constexpr int kHeadSets = 8;   // counter sets: one per frame in flight (its sample launches follow one another on one
                               // stream and share it), reused round-robin
constexpr int kFaccSets = 4;   // colour-sum buffers (spp > 1): one per frame, reused round-robin

// The device buffers of the context's launches, their events and flags: made at the first launch, gone with every svo_resize
// (persist_free).  What must outlive a resize is in PersistSettings / PersistLimits (svo_persist_plan.h).
struct PersistBuffers {
  uint32_t *heads = nullptr;
  // a counter set / colour-sum buffer may still be in use by a frame in flight on another stream when the ring
  // comes round: the launch that re-uses it first waits (on the GPU, hipStreamWaitEvent) for the event its
  // previous user recorded
  hipEvent_t head_done[kHeadSets] = {};
  bool head_used[kHeadSets] = {};
  float *facc[kFaccSets] = {};
  hipEvent_t facc_done[kFaccSets] = {};
  bool facc_used[kFaccSets] = {};
  size_t facc_floats = 0;   // floats in each colour-sum buffer
  float *rc[kHeadSets] = {};   // row / column tables, one buffer per counter set (a set's launches are ordered by its event)
  size_t rc_floats = 0;        // floats in each
  uint32_t *prec[kHeadSets] = {};   // path records of the spare-ray kernel, one buffer per counter set
  size_t prec_words = 0;
  uint4 *prim[kHeadSets] = {};      // primary-hit records of persist_span_kernel's lanes, one buffer per counter set
  size_t prim_waves = 0;            // persistent waves each of them has room for
  // The primary-hit cache (persist_kept_kernel): ONE buffer for the context, whatever counter set a launch runs on.  What a
  // primary hit depends on is its key; a launch whose key equals the cache's reads it once the fill has been SEEN complete
  // (hipEventQuery; nothing here ever waits), a launch with another key fills it once the buffer is idle -- the last fill and
  // every launch that read it seen complete -- and every other launch runs persist_span_kernel as before.
  struct KeptKey {
    const uint8_t *pool; const uint2 *desc;
    uint64_t pool_epoch;
    uint32_t pool_len, cam[15];
    int32_t width, height, y0, y1, row_step, out_y0, tiles_y;
  };
  uint4 *kept = nullptr;
  size_t kept_cap = 0;         // records per plane the buffer has room for
  size_t kept_failed = 0;      // ... and the size hipMalloc last refused: launches of that size and larger stay on persist_span_kernel
  KeptKey kept_key = {};
  bool kept_valid = false;     // kept_key describes the last fill (cleared by persist_kept_drop)
  bool kept_fill_inflight = false;   // a fill was launched and kept_filled not yet seen complete
  hipEvent_t kept_filled = nullptr;
  bool kept_reader[kHeadSets] = {};  // the set's head_done is behind a launch that read the cache (or behind one that waited for it)
  // the ray records of the dense pass (bounce_rays_kernel -> persist_cast_kernel), one buffer per counter set like the tables:
  // ray_record_bytes() x ray_records each, the 16-byte plane first
  uint8_t *rays[kHeadSets] = {};
  size_t ray_records = 0;      // records each has room for
  size_t rays_failed = 0;      // ... and the size hipMalloc last refused: launches of that size and larger shade in persist_kept_kernel<false>
  int last_thresh = 9, last_blocks = 0, last_per_cu = 0;   // shape of the last launch (svo_launch_info)
  unsigned launches = 0, frames = 0;
};

// everything the persistent pipeline keeps for a context
struct PersistState {
  PersistSettings set;
  PersistLimits lim;
  PersistBuffers buf;
};

inline void persist_free(PersistBuffers &b) {
  if (b.heads) (void)hipFree(b.heads);
  for (auto &p : b.prec) if (p) (void)hipFree(p);
  for (auto &p : b.rc) if (p) (void)hipFree(p);
  for (auto &p : b.prim) if (p) (void)hipFree(p);
  for (auto &p : b.rays) if (p) (void)hipFree(p);
  for (auto &f : b.facc) if (f) (void)hipFree(f);
  for (auto &e : b.head_done) if (e) (void)hipEventDestroy(e);
  for (auto &e : b.facc_done) if (e) (void)hipEventDestroy(e);
  if (b.kept) (void)hipFree(b.kept);
  if (b.kept_filled) (void)hipEventDestroy(b.kept_filled);
  b = PersistBuffers();
}

// the cache describes nothing any more (the pool changed, the host opted out).  The buffer and what is known about the launches
// still using it stay: the next fill waits its turn like any other.
inline void persist_kept_drop(PersistBuffers &b) { b.kept_valid = false; }
// the pool's contents change: the epoch is part of the cache's key, and the cache is empty from here on
inline void persist_pool_changed(PersistState &p) { p.set.pool_epoch++; persist_kept_drop(p.buf); }

// has `ev` completed?  Never waits; hipErrorNotReady is no error and does not stay behind as one.
inline bool persist_event_done(hipEvent_t ev) {
  const hipError_t e = hipEventQuery(ev);
  if (e == hipErrorNotReady) (void)hipGetLastError();
  return e == hipSuccess;
}
// has the last fill been seen complete?  (true when there never was one)
inline bool persist_kept_filled(PersistBuffers &b) {
  if (b.kept_fill_inflight && persist_event_done(b.kept_filled)) b.kept_fill_inflight = false;
  return !b.kept_fill_inflight;
}
// ... and every launch that read the cache?
inline bool persist_kept_idle(PersistBuffers &b) {
  if (!persist_kept_filled(b)) return false;
  bool idle = true;
  for (int i = 0; i < kHeadSets; i++) {
    if (b.kept_reader[i] && persist_event_done(b.head_done[i])) b.kept_reader[i] = false;
    idle = idle && !b.kept_reader[i];
  }
  return idle;
}

// The row / column tables of a launch: per frame of the batch W + H threads.  A handful of workgroups: unlike a kernel of one
// thread per pixel (tried and dropped, profiles/round5_experiments.txt) they find their slots next to the persistent waves of the
// launches in flight as soon as a few of those retire.  The same device functions primary_direction_cam / pixel_rand call, on the
// same values, in the same order.
// Workgroups of ONE wave: a workgroup of four needs four free wave slots on one CU at the same moment, which CUs packed with
// persistent waves offer much later than the single slot a lone wave needs.
#ifndef SVO_RC_BLOCK
#define SVO_RC_BLOCK 64
#endif
#ifndef SVO_RC_WAVES
#define SVO_RC_WAVES 4    // workgroups per frame of the launch
#endif
// the counter set of a launch without tables: zeroed by a one-wave kernel (hipMemsetAsync is a fill kernel of wider workgroups here)
__global__ __launch_bounds__(64) void zero_words_kernel(uint32_t *p, const uint32_t n) {
  for (uint32_t w = threadIdx.x; w < n; w += 64u) p[w] = 0u;
}
constexpr int kCamPack = 8;   // per-frame cameras of a launch that travel in the table kernel's arguments (no copy in front of it)
struct FrameVarPack { FrameVar v[kCamPack]; };
__global__ __launch_bounds__(SVO_RC_BLOCK) void rc_table_kernel(const Frame f, FrameVar *fvar, float *rc, const uint32_t stride, const int sample,
                                                                uint32_t *heads, const FrameVarPack pack, const int npack) {
  // (the launch's counter set is zeroed here too: one small kernel in front of the launch instead of a fill kernel and this one;
  // and with npack > 0 the launch's per-frame cameras arrive in `pack` and are written to the slot's table `fvar`, which the
  // persistent kernel reads with a scalar load per frame: no host-to-device copy -- a blit kernel on this runtime -- in front either)
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (uint32_t w = threadIdx.x; w < (uint32_t)kHeadWords; w += (uint32_t)SVO_RC_BLOCK) heads[w] = 0u;
    for (uint32_t w = threadIdx.x; w < (uint32_t)npack * 16u; w += (uint32_t)SVO_RC_BLOCK)
      ((uint32_t *)fvar)[w] = ((const uint32_t *)pack.v)[w];
  }
  const int k = (int)blockIdx.y;
  float *fr = rc + (size_t)k * stride;
  const float *cam = npack > 0 ? pack.v[k].cam : (fvar ? fvar[k].cam : f.cam);
  const float seed2 = (float)((npack > 0 ? pack.v[k].frame_number : (fvar ? fvar[k].frame_number : f.frame_number + k)) + sample);
  const float k0 = 0.1f * 78.233f, k1 = 0.02f * 78.233f;   // (pixel_rand's folded constants)
  // a few waves per frame, each over a strided share of the W + H entries: the fewer workgroups, the sooner all of them have a slot
  for (int i = (int)(blockIdx.x * (uint32_t)SVO_RC_BLOCK + threadIdx.x); i < f.width + f.height; i += (int)(gridDim.x * (uint32_t)SVO_RC_BLOCK)) {
    if (i < f.width) {
      const float x = (float)i;
      fr[2 * i] = rand_of_dot(x * 12.9898f + seed2 * k0);
      fr[2 * i + 1] = (x + 0.5f) / (float)f.width;
    } else {
      const int y = i - f.width;
      const float v = ((float)y + 0.5f) / (float)f.height;
      float *row = fr + ((2 * f.width + 3) & ~3) + 8 * y;
      row[0] = mix_g(cam[3], cam[6], v); row[1] = mix_g(cam[4], cam[7], v); row[2] = mix_g(cam[5], cam[8], v);
      row[3] = rand_of_dot((float)y * 12.9898f + seed2 * k1);
      row[4] = mix_g(cam[9], cam[12], v); row[5] = mix_g(cam[10], cam[13], v); row[6] = mix_g(cam[11], cam[14], v);
      row[7] = 0.0f;
    }
  }
}

// the spare-ray kernel (variants/svo_persist2.hip.h, included behind this file by svo_hip.hip in SVO_VARIANTS builds)
#ifndef SVO_VARIANTS
#define SVO_VARIANTS 0
#endif
#define SVO_HAVE_SPARE (SVO_ASM_LOOP && SVO_VARIANTS)
#if SVO_HAVE_SPARE
template <int kMode>
inline void persist2_launch_mode(const PersistArgs &a, int blocks, hipStream_t stream);
inline hipError_t persist2_occupancy(int *per_cu);
#endif
// SVO_SPARE_RECORDS: 0 = the two path records of a lane live in registers (18 each; the kernel then runs 4 waves per SIMD),
// 1 = in global memory (6 waves per SIMD; measured: the records' traffic -- 144 bytes per ray written and read back, more
// than the caches hold with six launches in flight -- costs more than the lanes gained: profiles/round5_experiments.txt)
#ifndef SVO_SPARE_RECORDS
#define SVO_SPARE_RECORDS 0
#endif

template <int kMode>
inline void persist_launch_mode(const PersistArgs &a, int blocks, hipStream_t stream) {
#if SVO_HAVE_SPARE
  if (a.spare) { persist2_launch_mode<kMode>(a, blocks, stream); return; }
#endif
  if (kMode == 0 && a.span) {   // (persist_plan: mode 0, one camera, the descriptor walk; any other mode runs its own kernel)
    if (a.kept) {   // (persist_plan: only with the tables)
      if (a.kept_fill) hipLaunchKernelGGL((persist_kept_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
      else hipLaunchKernelGGL((persist_kept_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
      return;
    }
    if (a.rc) hipLaunchKernelGGL((persist_span_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((persist_span_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    return;
  }
  if (a.rc && a.desc) {   // (the tables are only made for launches that walk the descriptor table)
    if (a.fvar) hipLaunchKernelGGL((persist_kernel<kMode, DescWalk, true, true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((persist_kernel<kMode, DescWalk, false, true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    return;
  }
  if (a.fvar) {
    if (a.desc) hipLaunchKernelGGL((persist_kernel<kMode, DescWalk, true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((persist_kernel<kMode, ByteWalk, true>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
  } else if (a.desc) hipLaunchKernelGGL((persist_kernel<kMode, DescWalk>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL((persist_kernel<kMode, ByteWalk>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
}

__global__ void persist_resolve_kernel(const Frame f, const float *facc, size_t npix, uint32_t *color) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = frame_gy(f, (int)blockIdx.y >> 3, (int)blockIdx.y & 7);
  if (x >= f.width || y >= f.y1 || y >= f.height) return;
  const size_t pix = (size_t)blockIdx.z * f.frame_stride +      // frame blockIdx.z of a batch
                     (size_t)frame_oy(f, (int)blockIdx.y >> 3, (int)blockIdx.y & 7) * f.width + x;
  const float inv = 1.0f / (float)f.spp;
  const V3 sum = mk(facc[pix], facc[npix + pix], facc[2 * npix + pix]);
  color[pix] = final_rgba8(f, x, y, mk(sum.x * inv, sum.y * inv, sum.z * inv), color + pix);
}

// The same for a launch that left every sample in a slot of its own (persist_emit, a.fold > 1): one workgroup per tile;
// the samples are added in sample order, the order in which one launch per sample adds them: ((0 + s0) + s1) + ...
__global__ __launch_bounds__(64) void persist_resolve_tiles_kernel(const Frame f, const float *facc, int fold, uint32_t *color) {
  const uint32_t l = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y, k = blockIdx.z;
  const float *p = facc + (((size_t)k * (size_t)f.ntiles + (size_t)ty * f.tiles_x + tx) * (size_t)fold) * 192 + l;
  V3 sum = mk(0.0f + p[0], 0.0f + p[64], 0.0f + p[128]);
  for (int i = 1; i < fold; i++) sum = mk(sum.x + p[192 * i], sum.y + p[192 * i + 64], sum.z + p[192 * i + 128]);
  const int x = (int)(tx * 8u + (l & 7u)), y = frame_gy(f, (int)ty, (int)(l >> 3));
  if (x >= f.width || y >= f.y1 || y >= f.height) return;
  const size_t pix = (size_t)k * f.frame_stride + (size_t)frame_oy(f, (int)ty, (int)(l >> 3)) * f.width + x;
  const float inv = 1.0f / (float)f.spp;
  color[pix] = final_rgba8(f, x, y, mk(sum.x * inv, sum.y * inv, sum.z * inv), color + pix);
}

// A progressive sequence (f.seq frames of the cross-frame accumulation in one launch, every frame's colour in a slot of its
// own like a sample): the reference's recurrence in frame order -- blend with the texel the previous frame left, quantise to
// rgba8 exactly as imageStore / imageLoad do (svotrace.comp:712-719, pins in svo_fused.hip.h::final_rgba8_v), next frame.
// What f.seq dispatches of one frame each would leave in the image, bit for bit; `color` holds the image the sequence starts on.
__global__ __launch_bounds__(64) void persist_resolve_sequence_kernel(const Frame f, const float *facc, int fold, uint32_t *color) {
  const uint32_t l = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
  const float *p = facc + (((size_t)ty * f.tiles_x + tx) * (size_t)fold) * 192 + l;
  const int x = (int)(tx * 8u + (l & 7u)), y = frame_gy(f, (int)ty, (int)(l >> 3));
  if (x >= f.width || y >= f.y1 || y >= f.height) return;
  const size_t pix = (size_t)frame_oy(f, (int)ty, (int)(l >> 3)) * f.width + x;
  uint32_t last = color[pix];
  for (int i = 0; i < fold; i++)
    last = final_rgba8_v(f, f.frame_number + i, x, y, mk(0.0f + p[192 * i], 0.0f + p[192 * i + 64], 0.0f + p[192 * i + 128]), last);
  color[pix] = last;
}

// the most bytes of sample slots one launch may ask for (persist_can_fold); a variants build reads the environment's, once
inline unsigned long long persist_fold_budget() {
#if SVO_VARIANTS
  static const unsigned long long budget = getenv("SVO_FOLD_BYTES") ? strtoull(getenv("SVO_FOLD_BYTES"), nullptr, 10) : kFoldBytes;
  return budget;
#else
  return kFoldBytes;
#endif
}

// What one launch is given besides its Frame.
struct PersistLaunch {
  const uint8_t *pool = nullptr;
  uint32_t *color = nullptr;
  float *depth = nullptr;
  uint4 *hits = nullptr;
  size_t out_npix = 0;   // elements of the output images: W*H, or more when packed stripes overhang the frame (caller-owned
                         // gather buffers); the colour-sum planes are indexed like the outputs
  hipStream_t stream = nullptr;
  LaunchShape shape = kPlain;   // who shares the GPU with the launch (svo_persist_plan.h) ...
  int overlap_sets = 0;         // ... kOverlap: the number of image sets taking turns
  // the interior-descriptor table of the pool (svo_derive.hip.h), or null = walk the records
  const uint2 *desc = nullptr, *aux = nullptr;
  uint32_t desc_count = 0;
  const float4 *ntab = nullptr;   // the context's normal table, or null = the kernels decode in place
  // fvar: where the launch's per-frame cameras live on the device (null: one camera, f.cam); fvar_host: the same on the host.  They
  // reach the device inside the table kernel's arguments when the launch has one and they fit (kCamPack), else through copy_cams
  // (the caller's staged copy on `stream`), called in front of the first kernel that reads them.
  FrameVar *fvar = nullptr;
  const FrameVar *fvar_host = nullptr;
  int (*copy_cams)(void *) = nullptr;
  void *copy_arg = nullptr;
};

// The buffers' first use: the counter sets and the events.  The context's first use: what the device offers, and in a
// variants build the experiment knobs of the environment (they override svo_set_tuning: libsvohip_variants.so only).
inline hipError_t persist_prepare(PersistState &p) {
  PersistBuffers &b = p.buf;
  hipError_t e;
  if (!b.heads) {
    if ((e = hipMalloc((void **)&b.heads, kHeadSets * kHeadWords * sizeof(uint32_t))) != hipSuccess) return e;
    for (auto &ev : b.head_done)
      if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    for (auto &ev : b.facc_done)
      if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
  }
  if (!p.lim.known) {
    int dev = 0, cus = 256, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel<0, ByteWalk>, 64, 0) != hipSuccess || per_cu < 1)
      per_cu = 16;
    p.lim.max_per_cu = per_cu;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel<0, DescWalk>, 64, 0) != hipSuccess || per_cu < 1)
      per_cu = 16;
    p.lim.max_per_cu_desc = per_cu;
    p.lim.cus = cus;
    p.lim.known = true;
#if SVO_VARIANTS
    PersistSettings &s = p.set;
    if (const char *e1 = getenv("SVO_PERSIST_WAVES_PER_CU")) s.waves_per_cu = atoi(e1);
    if (const char *e2 = getenv("SVO_PERSIST_THRESH")) s.thresh_num = atoi(e2);
    if (const char *e3 = getenv("SVO_SPARE")) s.spare_mode = atoi(e3) != 0 ? 1 : 0;
    if (const char *e4 = getenv("SVO_RC_TABLE")) s.table_mode = atoi(e4) != 0 ? 1 : 0;
    if (const char *e5 = getenv("SVO_NORMAL_TABLE")) s.ntab_mode = atoi(e5) != 0 ? 1 : 0;
    if (const char *e6 = getenv("SVO_BATCH_PRIMARY")) s.span_mode = atoi(e6) != 0 ? 1 : 0;
    if (const char *e7 = getenv("SVO_DENSE_SHADE")) s.dense_mode = atoi(e7) != 0 ? 1 : 0;
    if (const char *e8 = getenv("SVO_RAY_LIST")) s.list_mode = atoi(e8) != 0 ? 1 : 0;
#endif
  }
  return hipSuccess;
}

// The primary-hit cache's say in a launch the plan names a candidate (`need` = plan.kept_records): a.kept and a.kept_fill when
// the launch reads or fills the cache, a.kept = null when it runs persist_span_kernel as before.  An allocation that fails is no
// error: launches of that size stay on today's kernel.
inline hipError_t persist_kept_choose(PersistState &p, const PersistLaunch &in, const Frame &f, size_t need, PersistArgs &a) {
  PersistBuffers &b = p.buf;
  PersistBuffers::KeptKey key;
  memset(&key, 0, sizeof key);
  key.pool = in.pool; key.desc = in.desc; key.pool_epoch = p.set.pool_epoch; key.pool_len = f.pool_len;
  memcpy(key.cam, f.cam, sizeof key.cam);
  key.width = f.width; key.height = f.height; key.y0 = f.y0; key.y1 = f.y1; key.row_step = f.row_step; key.out_y0 = f.out_y0;
  key.tiles_y = f.tiles_y;
  if (b.kept_valid && memcmp(&key, &b.kept_key, sizeof key) == 0) {
    if (persist_kept_filled(b)) a.kept = b.kept;
  } else if ((b.kept_failed == 0 || need < b.kept_failed) && need < (1ull << 30) && persist_kept_idle(b)) {
    b.kept_valid = false;
    if (!b.kept_filled && hipEventCreateWithFlags(&b.kept_filled, hipEventDisableTiming) != hipSuccess) {
      b.kept_filled = nullptr;
      (void)hipGetLastError();
    } else if (b.kept_cap < need) {   // (idle, so nothing reads the old buffer; the wait is the one `prim` grows behind)
      hipError_t e;
      if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
      if (b.kept) (void)hipFree(b.kept);
      b.kept = nullptr; b.kept_cap = 0;
      if (hipMalloc((void **)&b.kept, 3 * need * sizeof(uint4)) == hipSuccess) b.kept_cap = need;
      else { b.kept = nullptr; b.kept_failed = need; (void)hipGetLastError(); }
    }
    if (b.kept_filled && b.kept_cap >= need) { a.kept = b.kept; a.kept_fill = 1; b.kept_key = key; }
  }
  a.kept_n = (uint32_t)b.kept_cap; a.kept_origin = (uint32_t)f.out_y0 * (uint32_t)f.width;
  return hipSuccess;
}
// ... and behind the launch on counter set `hset`: a fill's event and key, a reader's mark on its set
inline hipError_t persist_kept_launched(PersistState &p, const PersistArgs &a, int hset, hipStream_t stream) {
  PersistBuffers &b = p.buf;
  if (a.kept && a.kept_fill) {
    const hipError_t e = hipEventRecord(b.kept_filled, stream);
    if (e != hipSuccess) return e;
    b.kept_valid = true; b.kept_fill_inflight = true; p.set.kept_fills++;
  } else if (a.kept) {
    b.kept_reader[hset] = true; p.set.kept_reuses++;
  }
  return hipSuccess;
}

// Does this launch take the dense pass?  The plan says it may (PersistPlan::dense), persist_kept_choose that it READS the cache; what
// is left is room for its ray records.  They grow with the FILL, next to the cache itself: the wait for the device and the
// allocations (8 ms at 1080p x 4 frames) then fall on the submission that casts its primaries anyway, not on the first one that
// could run without.  An allocation that fails is no error: launches of that size shade in their rounds as before.
inline hipError_t persist_dense_choose(PersistState &p, const PersistPlan &plan, const PersistArgs &a, int hset, RayArgs &ra, RayListArgs &rl) {
  PersistBuffers &b = p.buf;
  ra.ray = nullptr; ra.hitc = nullptr; ra.n = 0;
  rl.ray = nullptr; rl.tag = nullptr;
  if (!plan.dense || !a.kept) return hipSuccess;
  if (b.ray_records < plan.ray_records) {
    if (b.rays_failed != 0 && plan.ray_records >= b.rays_failed) return hipSuccess;
    // (launches in flight may still read the old records: grow_device_buffers waits for the device)
    const hipError_t e = grow_device_buffers(b.rays, nullptr, b.ray_records, plan.ray_records, plan.ray_records * ray_record_bytes(p.set.list_mode != 0));
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      for (auto &r : b.rays) { if (r) (void)hipFree(r); r = nullptr; }
      b.rays_failed = plan.ray_records;
      return hipSuccess;
    }
    if (e != hipSuccess) return e;
  }
  if (a.kept_fill) return hipSuccess;
  if (plan.list) {
    rl.ray = (uint4 *)b.rays[hset];
    rl.tag = (uint2 *)(b.rays[hset] + b.ray_records * sizeof(uint4));
    return hipSuccess;
  }
  ra.ray = (uint4 *)b.rays[hset];
  ra.hitc = (uint32_t *)(b.rays[hset] + b.ray_records * sizeof(uint4));
  ra.n = (uint32_t)plan.kept_records;
  return hipSuccess;
}

// the kernels' arguments, for a launch on counter set `hset` (a.reverse and a.sample: per kernel launch; the cache: persist_kept_choose)
inline PersistArgs persist_args(const PersistPlan &plan, const Frame &f, const PersistLaunch &in, const PersistBuffers &b, int hset, float *facc) {
  PersistArgs a;
  a.pool = in.pool; a.f = f; a.color = in.color; a.depth = in.depth; a.hits = in.hits; a.facc = facc; a.npix = plan.npix;
  a.heads = b.heads + (size_t)hset * kHeadWords;
  a.tiles_per_band = (f.ntiles + 7) / 8;
  a.rows_per_band = plan.rows_per_band;
  a.reverse = 0; a.sample = 0;
  a.thresh_num = plan.thresh_num;
  a.fold = plan.fold;
  a.group = kFoldGroup;
  memcpy(a.mg_rows, plan.mg_rows, sizeof a.mg_rows);
  memcpy(a.mg_tpf, plan.mg_tpf, sizeof a.mg_tpf);
  a.desc = in.desc; a.aux = in.aux; a.desc_count = in.desc_count;
  a.fvar = in.fvar;
  // (a counter set's launches are ordered by the set's event: so are its path records, primary-hit records and tables)
  a.prec = (plan.spare && SVO_SPARE_RECORDS) ? b.prec[hset] : nullptr;
  a.spare = plan.spare ? 1 : 0;
  a.span = plan.span ? 1 : 0;
  a.prim = plan.span ? b.prim[hset] : nullptr;
  a.rc = plan.tables ? b.rc[hset] : nullptr;
  a.rc_stride = (uint32_t)plan.rc_stride;
  a.ntab = in.ntab;
  a.kept = nullptr; a.kept_n = 0; a.kept_origin = 0; a.kept_fill = 0;
  return a;
}

// the colour sums of a launch become rgba8: by plane, by tile (folded samples) or frame after frame (a folded sequence)
inline void persist_resolve(const PersistPlan &plan, const Frame &f, const PersistLaunch &in, const float *facc) {
  const unsigned nb = (unsigned)(f.batch > 1 ? f.batch : 1);
  if (plan.resolve == PersistPlan::kSequence) {
    hipLaunchKernelGGL(persist_resolve_sequence_kernel, dim3((unsigned)f.tiles_x, (unsigned)f.tiles_y), dim3(64), 0, in.stream, f, facc, plan.fold, in.color);
  } else if (plan.resolve == PersistPlan::kTiles) {
    hipLaunchKernelGGL(persist_resolve_tiles_kernel, dim3((unsigned)f.tiles_x, (unsigned)f.tiles_y, nb), dim3(64), 0, in.stream, f, facc, plan.fold, in.color);
  } else {
    dim3 grid((unsigned)((f.width + 255) / 256), (unsigned)(f.tiles_y * 8), nb);
    hipLaunchKernelGGL(persist_resolve_kernel, grid, dim3(256), 0, in.stream, f, facc, plan.npix, in.color);
  }
}

// One frame (or batch, or folded sequence) of `f` as `in` says: what is launched is persist_plan's decision, made here once.
inline int persist_launch(PersistState &p, const Frame &f, const PersistLaunch &in) {
  PersistBuffers &b = p.buf;
  hipError_t e;
  if ((e = persist_prepare(p)) != hipSuccess) return (int)e;
  const bool has_table = in.desc != nullptr;
#if SVO_HAVE_SPARE
  if (persist_uses_spare(p.set, has_table, true) && p.lim.max_per_cu_spare == 0) {
    int per_cu = 0;
    if (persist2_occupancy(&per_cu) != hipSuccess || per_cu < 1) per_cu = 16;
    p.lim.max_per_cu_spare = per_cu;
  }
#endif
  const PersistPlan plan = persist_plan(p.set, p.lim, f, in.shape, in.overlap_sets, has_table, in.fvar != nullptr, SVO_HAVE_SPARE != 0,
                                        in.out_npix, persist_fold_budget());
  if (plan.spare && SVO_SPARE_RECORDS) {
    const size_t need = (size_t)p.lim.cus * (size_t)p.lim.max_per_cu_desc * (size_t)(2 * 18 * 64);   // = kRecWaveWords per wave that fits
    if (b.prec_words < need && (e = grow_device_buffers(b.prec, nullptr, b.prec_words, need, need * sizeof(uint32_t))) != hipSuccess)
      return (int)e;
  }
  b.last_per_cu = plan.per_cu;
  const unsigned frame_no = b.frames++;
  if (plan.invalid) return (int)hipErrorInvalidValue;
  const bool resolve = plan.resolve != PersistPlan::kNone;
  float *facc = nullptr;
  int fset = 0;
  if (resolve) {   // grow: nothing may still be summing into the old buffers
    if (b.facc_floats < plan.facc_floats &&
        (e = grow_device_buffers(b.facc, b.facc_used, b.facc_floats, plan.facc_floats, plan.facc_floats * sizeof(float))) != hipSuccess)
      return (int)e;
    fset = (int)(frame_no % kFaccSets);
    facc = b.facc[fset];
    if (b.facc_used[fset] && (e = hipStreamWaitEvent(in.stream, b.facc_done[fset], 0)) != hipSuccess) return (int)e;
  }
  b.last_thresh = plan.thresh_num;
  b.last_blocks = plan.blocks;
  // (launches in flight may still use the old records)
  if (plan.span && b.prim_waves < (size_t)plan.blocks &&
      (e = grow_device_buffers(b.prim, nullptr, b.prim_waves, plan.prim_waves, plan.prim_waves * 64 * kSpanWords * sizeof(uint32_t))) != hipSuccess)
    return (int)e;
  // a ring of counter sets: frames may be in flight on different streams at the same time.  A frame's sample launches
  // are ordered by its stream, so they share the frame's set; only another frame's re-use waits (for the event)
  const int hset = (int)(frame_no % kHeadSets);
  // (one wait for the device, not one per set inside a run; launches in flight may still read the old tables)
  if (plan.tables && b.rc_floats < plan.rc_floats &&
      (e = grow_device_buffers(b.rc, nullptr, b.rc_floats, plan.rc_floats, plan.rc_floats * sizeof(float))) != hipSuccess)
    return (int)e;

  PersistArgs a = persist_args(plan, f, in, b, hset, facc);
  if (p.set.ntab_mode == 0) a.ntab = nullptr;
  if (plan.cache && (e = persist_kept_choose(p, in, f, plan.kept_records, a)) != hipSuccess) return (int)e;
  RayArgs ra;
  RayListArgs rl;
  if ((e = persist_dense_choose(p, plan, a, hset, ra, rl)) != hipSuccess) return (int)e;

  if (b.head_used[hset] && (e = hipStreamWaitEvent(in.stream, b.head_done[hset], 0)) != hipSuccess) return (int)e;
  const int nb = f.batch > 1 ? f.batch : 1;
  for (int s = 0; s < plan.launches; s++) {
    a.reverse = (int)(b.launches++ & 1u);   // serpentine: consecutive launches walk the columns in opposite directions
    a.sample = s;
    const bool packed = a.rc && in.fvar && in.fvar_host && nb <= kCamPack;
    if (in.fvar && !packed && s == 0 && in.copy_cams) { const int rcc = in.copy_cams(in.copy_arg); if (rcc) return rcc; }
    if (a.rc) {
      FrameVarPack pack;
      if (packed) memcpy(pack.v, in.fvar_host, (size_t)nb * sizeof(FrameVar));
      else memset(&pack, 0, sizeof pack);
      const unsigned per_frame = (unsigned)((f.width + f.height + SVO_RC_BLOCK - 1) / SVO_RC_BLOCK);
      const dim3 tgrid(per_frame < (unsigned)SVO_RC_WAVES ? per_frame : (unsigned)SVO_RC_WAVES, (unsigned)nb);
      hipLaunchKernelGGL(rc_table_kernel, tgrid, dim3(SVO_RC_BLOCK), 0, in.stream, f, in.fvar, b.rc[hset], a.rc_stride, s, a.heads, pack, packed ? nb : 0);
    } else {
      hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, in.stream, a.heads, (uint32_t)kHeadWords);
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (rl.ray) {   // the same with the rays to cast as a list
      hipLaunchKernelGGL(ray_list_kernel, dim3((unsigned)f.tiles_x, (unsigned)f.tiles_y), dim3(64), 0, in.stream, a, rl);
      if ((e = hipGetLastError()) != hipSuccess) return (int)e;
      hipLaunchKernelGGL(persist_runs_kernel, dim3((unsigned)plan.blocks), dim3(64), 0, in.stream, a, rl);
      if ((e = hipGetLastError()) != hipSuccess) return (int)e;
      p.set.dense_launches++;
      continue;
    }
    if (ra.ray) {   // (mode 0, one launch: persist_plan) the tables -> every (pixel, frame)'s shading -> the casts
      hipLaunchKernelGGL(bounce_rays_kernel, dim3((unsigned)f.tiles_x, (unsigned)f.tiles_y, (unsigned)nb), dim3(64), 0, in.stream, a, ra);
      if ((e = hipGetLastError()) != hipSuccess) return (int)e;
      hipLaunchKernelGGL(persist_cast_kernel, dim3((unsigned)plan.blocks), dim3(64), 0, in.stream, a, ra);
      if ((e = hipGetLastError()) != hipSuccess) return (int)e;
      p.set.dense_launches++;
      continue;
    }
    switch (f.render_mode) {
      case 0: persist_launch_mode<0>(a, plan.blocks, in.stream); break;
      case 1: persist_launch_mode<1>(a, plan.blocks, in.stream); break;
      case 2: persist_launch_mode<2>(a, plan.blocks, in.stream); break;
      case 3: persist_launch_mode<3>(a, plan.blocks, in.stream); break;
      default: persist_launch_mode<4>(a, plan.blocks, in.stream); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  if ((e = hipEventRecord(b.head_done[hset], in.stream)) != hipSuccess) return (int)e;
  b.head_used[hset] = true;
  if ((e = persist_kept_launched(p, a, hset, in.stream)) != hipSuccess) return (int)e;
  if (resolve) {
    persist_resolve(plan, f, in, facc);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipEventRecord(b.facc_done[fset], in.stream)) != hipSuccess) return (int)e;
    b.facc_used[fset] = true;
  }
  return 0;
}

}  // namespace svo
