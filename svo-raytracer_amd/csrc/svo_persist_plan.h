// svo_persist_plan.h -- what a launch of the persistent pipeline (svo_persistent.hip.h) decides before it touches the GPU:
// which kernel, how many waves, whether samples fold, whether the batch shares its primary rays, whether tables are made,
// whether the primary-hit cache is a candidate, whether its readers shade in a dense pass, and how much room the launch's buffers need.  A pure function of a few
// integers: no HIP call, no environment, no device type -- a host compiler can include this header on its own
// (tests/persist_plan_cases.cpp prints the plan of a list of cases).
#pragma once
#include "svo_kernels.h"

#include <stddef.h>
#include <stdint.h>

namespace svo {

// Who else is on the GPU while the launch runs: nobody the library knows of, the other slots of a ring (svo_ring_*), or
// the other image sets svo_dispatch_async takes turns on.
enum LaunchShape { kPlain, kRing, kOverlap };

// Persistent waves per CU and launch when several launches share the GPU (a ring of more than one slot): the next launch's
// waves take the CUs the previous launch's tail frees.  Swept in rounds 2-4 (profiles/round4_experiments.txt: 10 waves with
// a round once at most 9/16 of the lanes are still traversing is the shape every headline number was measured on; 16 waves: -6 %).
constexpr int kRingWavesPerCu = 10;
// ... and when svo_dispatch_async takes turns on n {stream, image} sets (the reference's loop: one frame per launch, up to n
// launches in flight): waves per CU and launch by n -- about 32 / n, the best of tools/loop_shape.py's sweeps
// (profiles/round6_experiments.txt: 2 sets 12, 3 sets 10, 4 sets 8, 5 and more 6)
inline int overlap_waves_per_cu(int sets) { return sets <= 2 ? 12 : sets == 3 ? 10 : sets == 4 ? 8 : 6; }

// PersistSettings::list_mode of a new context
#ifndef SVO_RAY_LIST
#define SVO_RAY_LIST 1
#endif
// the round threshold of the spare-ray kernel (variants/svo_persist2.hip.h), sixteenths
#ifndef SVO_SPARE_THRESH
#define SVO_SPARE_THRESH 13
#endif
constexpr uint32_t kSpanWords = 12;   // words per persistent lane of a kSpan launch's primary-hit record: three uint4, [wave][3][lane]
constexpr unsigned long long kFoldBytes = 4ull << 30;   // the most sample slots one launch may ask for

// What the host set for the context's lifetime (svo_set_tuning, svo_set_primary_cache, svo_set_reserved_cus; in a variants
// build the SVO_* environment, read once), and the counts svo_primary_cache_info reports.  Nothing here dies with svo_resize.
struct PersistSettings {
  int waves_per_cu = 0;   // 0 = automatic: as many as fit (PersistLimits) for one launch at a time, kRingWavesPerCu / overlap_waves_per_cu
                          // when the launch shares the GPU (LaunchShape)
  int thresh_num = 0;     // sixteenths; 0 = the running kernel's default: 9 for persist_kernel (8 / 9 / 10 / 11: 4.28 / 4.38 / 4.33 /
                          // 4.14 Grays/s, tools/history/sweep8.sh), SVO_SPARE_THRESH for the spare-ray kernel
  int spare_mode = 0;     // 1 = the spare-ray kernel (variants/svo_persist2.hip.h) on walkable pools (environment SVO_SPARE=1: round 5's
                          // experiment, measured slower than persist_kernel with launches in flight); 0 = persist_kernel everywhere
  int table_mode = 1;     // 1 = row / column tables + the kTab kernels where they apply (environment SVO_RC_TABLE=0: all in the rounds)
  int ntab_mode = 1;      // 1 = normals from the context's table; environment SVO_NORMAL_TABLE=0: decode in place
  int span_mode = 1;      // 1 = a static-camera batch of mode 0 casts its primary rays once (persist_span_kernel); environment
                          // SVO_BATCH_PRIMARY=0: every frame of the batch casts its own
  int kept_mode = 1;      // svo_set_primary_cache
  int dense_mode = 1;     // 1 = a launch that reads the cache and ends its paths with the bounce shades every (pixel, frame) in a dense
                          // pass and casts the prepared rays (bounce_rays_kernel + persist_cast_kernel); environment
                          // SVO_DENSE_SHADE=0: persist_kept_kernel<false> shades in its rounds
  int list_mode = SVO_RAY_LIST;   // 1 = the dense pass leaves a compact list of the rays to cast and the cast kernel draws runs of its
                          // entries (ray_list_kernel + persist_runs_kernel); 0 = a record per (frame, pixel), a slot per pixel
                          // (bounce_rays_kernel + persist_cast_kernel: the pass as it was first built, kept as the comparator).
                          // On: -6.5 % on the headline (profiles/ray_list.md).  Environment SVO_RAY_LIST in the variants build
  int cus_reserved = 0;   // CUs the launching stream may not use (svo_set_reserved_cus): fewer persistent waves
  uint64_t pool_epoch = 0;   // bumped by everything that changes the pool (svo_hip.hip::pool_changed)
  uint64_t kept_fills = 0, kept_reuses = 0;
  uint64_t dense_launches = 0;   // launches that took the dense pass (svo_dense_shade_info)
};

// What the device offers, asked once: CUs, and resident waves per CU of the record walk / the descriptor walk / the spare-ray kernel
struct PersistLimits {
  bool known = false;
  int cus = 256;
  int max_per_cu = 16, max_per_cu_desc = 16;
  int max_per_cu_spare = 0;   // 0 = not asked yet (only launches of that kernel ask)
};

// n / d by multiply-high with m = ceil(2^32 / d) = (2^32 + e) / d, 0 <= e < d: with n = q d + r the product is
// q 2^32 + q e + r (2^32 + e) / d, so the high word is q exactly while e (n + d) < 2^32.  That is checked against the largest n
// the launch can form (tile slots of a band x frames x samples: a 4K batch of 17 frames, or 1080p with 16 samples x 2 frames,
// is already past it); m = 0 otherwise = a real division (udiv_by).
inline uint32_t udiv_magic(uint32_t d, uint64_t n_max) {
  if (d <= 1u) return 0u;
  const uint32_t m = 0xffffffffu / d + 1u;
  const uint64_t e = (uint64_t)m * d - (1ull << 32);
  return e * (n_max + d) < (1ull << 32) ? m : 0u;
}

// ---------------- the draw of the persistent kernels, its pure half: band -> slots, slot -> tile, tile -> pixel.  Plain integers in,
// plain integers out, the same text on the device and on the host (tests/persist_draw_cases.cpp walks every slot of a launch
// through it).  On the device persist_cast_body (svo_persistent.hip.h) decodes its slots with it, a slot per pixel; the
// kernels at their register limit -- persist_body, persist_reuse_body, the spare-ray kernel -- write the same arithmetic
// out in their refill ("The dense pass", says what calling it cost them) and share udiv_by only.

// n / d by multiply-high with the reciprocal m of udiv_magic; m = 0: n is past what the reciprocal is exact for = a real division
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline uint32_t udiv_by(uint32_t n, uint32_t d, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return d <= 1u ? n : (m == 0u ? n / d : __umulhi(n, m));
#else
  return d <= 1u ? n : (m == 0u ? n / d : (uint32_t)(((uint64_t)n * m) >> 32));
#endif
}

// A band = a strip of whole tile rows, one per XCD, walked column by column: the pixels in flight on an XCD form a compact block
// of the screen (strip height x a few dozen tile columns) instead of two or three full-width tile rows.
struct Band {
  int first_row, rows;   // tile rows of the launch the band holds: rows_per_band of them, fewer in the last band, 0 behind it
  uint32_t frame;        // pixel slots of the band in one frame
  uint32_t total;        // slots to draw: over the launch's frames x samples, or (slot_is_pixel) one per pixel with all its frames
};
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline Band band_of(uint32_t band, int rows_per_band, int tiles_x, int tiles_y, int batch, int fold, bool slot_is_pixel) {
  Band b;
  b.first_row = (int)band * rows_per_band;
  int band_rows = tiles_y - b.first_row;
  band_rows = band_rows < 0 ? 0 : (band_rows > rows_per_band ? rows_per_band : band_rows);
  b.rows = band_rows;
  b.frame = (uint32_t)(band_rows * tiles_x) * 64u;
  b.total = slot_is_pixel ? b.frame : b.frame * (uint32_t)(batch * fold);
  return b;
}

// Slot of a band -> frame of the batch, sample, tile and lane in the tile.  Frames of a batch follow one another inside the band: a
// wave that runs out of frame k goes on with k + 1; the samples of a pixel (fold > 1) follow one another group by group of `group`
// tiles: sample 0 of the group's tiles, sample 1 of them, ... -- what is in flight at any time are a few tiles' samples, whose
// primary rays are the same and whose slots in the sample buffer are neighbours.  The two divisions -- by the band's tile slots per
// frame and by its tile rows -- are multiply-highs by reciprocals made on the host (mg_tpf, mg_rows: persist_plan).
struct SlotTile {
  uint32_t fi, si;       // frame of the batch (0 when a slot is a pixel), sample
  int tile_x, tile_y;    // tile of the launch
  uint32_t l;            // pixel of the tile, row-major
};
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline SlotTile slot_tile(const Band &b, uint32_t slot, int rows_per_band, int tiles_x, int reverse, const uint32_t *mg_rows, const uint32_t *mg_tpf,
                                 int batch, int fold, int group, bool slot_is_pixel) {
  SlotTile s;
  s.l = slot & 63u;
  const uint32_t per_frame = b.frame * (uint32_t)fold;
  const uint32_t tiles_pf = per_frame >> 6;   // tile slots of the band per frame
  const int last = b.rows == rows_per_band ? 0 : 1;   // which reciprocal of a pair: 0 = a full band, 1 = the one that is not
  s.fi = !slot_is_pixel && batch > 1 ? udiv_by(slot >> 6, tiles_pf, mg_tpf[last]) : 0u;
  const uint32_t q = (slot - s.fi * per_frame) >> 6;
  s.si = 0u;
  int j = (int)q;
  if (fold > 1) {
    const uint32_t tiles = b.frame >> 6, g = q / ((uint32_t)group * (uint32_t)fold);
    const uint32_t first = g * (uint32_t)group;
    const uint32_t gsize = tiles - first < (uint32_t)group ? tiles - first : (uint32_t)group;
    const uint32_t r = q - first * (uint32_t)fold;
    s.si = r / gsize;
    j = (int)(first + r % gsize);
  }
  int tile_x = (int)udiv_by((uint32_t)j, (uint32_t)b.rows, mg_rows[last]);
  s.tile_y = b.first_row + (j - tile_x * b.rows);
  if (reverse) tile_x = tiles_x - 1 - tile_x;   // serpentine: this launch ends where the next one starts
  s.tile_x = tile_x;
  return s;
}

// ... -> the pixel and its index in the output images; `inside` = false: the tile overhangs the frame or the launch's rows there
struct SlotPixel {
  int px, py;
  uint32_t pix;
  bool inside;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline SlotPixel slot_pixel(const Frame &f, const SlotTile &s) {
  SlotPixel p;
  p.px = s.tile_x * 8 + (int)(s.l & 7u);
  p.py = frame_gy(f, s.tile_y, (int)(s.l >> 3));
  p.inside = p.px < f.width && p.py < f.y1 && p.py < f.height;
  p.pix = s.fi * f.frame_stride + (uint32_t)frame_oy(f, s.tile_y, (int)(s.l >> 3)) * (uint32_t)f.width + (uint32_t)p.px;
  return p;
}

// ---------------- the ray list of the dense pass (PersistPlan::list: ray_list_kernel -> persist_runs_kernel, svo_persistent.hip.h), its pure half.
// The ray records of a launch are a compact list per band: only the (pixel, frame)s that cast a ray have an entry, in no
// particular order: a tile's wave appends its entries where the band's fill count stands.
// A record = {direction.xyz, rgba8 on a miss} in a 16-byte plane and {rgba8 on a hit, cache index | frame << kRayIndexBits} in an
// 8-byte plane: the cast kernel takes the output index and the origin (the kept hit's position) from the last word.
constexpr size_t kRayBytes = 20;       // a ray record at [frame][pixel]: {direction, rgba8 of a miss} in a 16-byte plane, rgba8 of a hit in a 4-byte plane
constexpr size_t kRayListBytes = 24;   // ... and an entry of the list
inline size_t ray_record_bytes(bool list) { return list ? kRayListBytes : kRayBytes; }
constexpr uint32_t kRayIndexBits = 24;                   // the pixel's index in the cache; the frame of the batch sits above it
constexpr uint32_t kRayIndexMask = (1u << kRayIndexBits) - 1u;
constexpr uint32_t kRayNoEntry = 0xffffffffu;            // no record's last word: a frame is below kRayMaxFrames
constexpr int kRayMaxFrames = 255;
// entries a wave of persist_runs_kernel reserves with one atomic on its band's draw cursor
// (128 / 256 / 512: 0.3417 / 0.2824 / 0.2825 ms per step, profiles/ray_list.md)
constexpr uint32_t kChunk = 256;

// do a launch's cache indices and frames fit a record's last word?  (persist_plan: if not, a context that keeps lists takes no dense pass)
inline bool ray_list_fits(size_t kept_records, int frames) {
  return kept_records <= (size_t)(kRayIndexMask + 1u) && frames <= kRayMaxFrames;
}

// Band `band`'s region of the launch's ray records: it starts at the record offset of the band's first tile row and has room for
// the band's pixels x frames.  The regions of the 8 bands tile tiles_y * 8 * width * frames records (PersistPlan::ray_records).
struct RayRegion {
  uint32_t first, room;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline RayRegion ray_region(uint32_t band, int rows_per_band, int tiles_y, int width, int frames) {
  const Band b = band_of(band, rows_per_band, 1, tiles_y, 1, 1, true);
  const uint32_t per_row = 8u * (uint32_t)width * (uint32_t)frames;   // records of one tile row
  RayRegion r;
  r.first = (b.rows > 0 ? (uint32_t)b.first_row : (uint32_t)tiles_y) * per_row;
  r.room = (uint32_t)b.rows * per_row;
  return r;
}

// The draw of persist_runs_kernel: a wave holds a run [cur, end) of its band's entries.  ray_run_reserve: what one atomicAdd of kChunk
// on the band's draw cursor (`base` = its return) gives a wave when the band holds `fill` entries; `last`: nothing of the band is
// left behind this run, the wave goes on to the next band once it is used up.  ray_run_take: how many of `idle` lanes get an
// entry (lane of rank r among the idle ones takes entry cur + r), and the run moves on.
struct RayRun {
  uint32_t cur, end;
  bool last;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline RayRun ray_run_reserve(uint32_t base, uint32_t fill) {
  RayRun r;
  r.cur = base < fill ? base : fill;
  r.end = base + kChunk < fill ? base + kChunk : fill;
  r.last = base + kChunk >= fill;
  return r;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
__attribute__((always_inline)) inline uint32_t ray_run_take(RayRun &r, uint32_t idle) {
  const uint32_t left = r.end - r.cur, n = idle < left ? idle : left;
  r.cur += n;
  return n;
}

// can `n` samples (or frames of a progressive sequence) per pixel be carried by one launch of `f`?
inline bool persist_can_fold(const Frame &f, int n, unsigned long long budget = kFoldBytes) {
  const unsigned long long nb = (unsigned long long)(f.batch > 1 ? f.batch : 1);
  const unsigned long long bytes = 192ull * (unsigned long long)n * (unsigned long long)f.ntiles * nb * sizeof(float);
  return n > 1 && f.bounces <= 255 && bytes <= budget && f.batch <= 255 && n < 65536 &&
         (long long)f.ntiles * (long long)nb * n < (1ll << 25);
}

// the spare-ray kernel walks the descriptor table in assembly: pools the table cannot state, and builds without it, run persist_kernel
inline bool persist_uses_spare(const PersistSettings &s, bool has_table, bool have_spare) {
  return have_spare && s.spare_mode != 0 && has_table;
}
// persistent waves per CU of a launch, of which `fit` are resident at most: the host's figure before the shape's
inline int persist_waves_per_cu(const PersistSettings &s, int fit, LaunchShape shape = kPlain, int overlap_sets = 0) {
  if (s.waves_per_cu > 0) return s.waves_per_cu;
  const int want = shape == kRing ? kRingWavesPerCu : (shape == kOverlap ? overlap_waves_per_cu(overlap_sets) : fit);
  return want < fit ? want : fit;
}
// a round starts once at most this many sixteenths of the lanes active at its start are still traversing
inline int persist_thresh(const PersistSettings &s, bool spare = false) {
  return s.thresh_num > 0 ? s.thresh_num : (spare ? SVO_SPARE_THRESH : 9);
}

struct PersistPlan {
  bool invalid = false;   // a progressive sequence that one launch cannot carry (the caller has checked persist_can_fold)
  bool spare = false;     // the spare-ray kernel
  int per_cu = 0, full_blocks = 0;   // waves per CU, and the waves that is on the CUs the launch may use
  int blocks = 0;         // ... capped by the launch's work
  int thresh_num = 9;
  // All samples of a frame in ONE launch when their slots fit (3 floats per pixel and sample): the launch's bands hold the
  // frame's samples one after the other like the frames of a batch, a wave goes from sample to sample without a tail, and the
  // sums cost one store per sample instead of a read-modify-write.  Otherwise one launch per sample.  Same bytes either way
  // (tests/test_gpu_inflight.py).
  int fold = 1;           // samples (frames of a sequence) per pixel carried by one launch
  int launches = 1;       // kernel launches: one, or one per sample
  bool sequence = false;
  enum Resolve { kNone, kPlanes, kTiles, kSequence } resolve = kNone;   // how the colour sums become rgba8
  bool span = false;      // a band slot is a pixel with all the frames of the batch (persist_span_kernel)
  int slot_frames = 1;    // frames a band's slots are counted over
  bool tables = false;    // row / column tables in front of the launch (the kTab kernels)
  bool cache = false;     // a candidate for the context's primary-hit cache (persist_kept_kernel)
  int rows_per_band = 0;  // tile rows per XCD band
  uint32_t mg_rows[2] = {0, 0}, mg_tpf[2] = {0, 0};   // PersistArgs: reciprocals for a full band and for the last one
  // room the launch needs
  size_t npix = 0;          // elements of a colour-sum plane: indexed like the outputs, a batch needs room for all its frames
  size_t facc_floats = 0;   // per colour-sum buffer (0: no resolve)
  size_t prim_waves = 0;    // persistent waves the primary-hit records must have room for (0: not a kSpan launch)
  size_t rc_stride = 0, rc_floats = 0;   // floats of one frame's tables / of the launch's (0: no tables)
  size_t kept_records = 0;  // records per plane of the cache: one per pixel of the rows the launch writes (0: no candidate)
  // a cache candidate whose paths are primary + one bounce: once the launch READS the cache, everything about a (pixel, frame)
  // but "did the bounce hit, and at what t" is known before its ray is cast, so the shading runs ahead of the walk in a dense
  // kernel.  (Longer paths shade their inner hits from the cast's result; every mirror mask is fine: scatter() takes it.)
  bool dense = false;
  size_t ray_records = 0;   // ray records the pass writes: one per (pixel of the launch's rows, frame of the batch) (0: no dense pass)
  bool list = false;        // ... as a compact list, that room cut into the bands' regions (ray_region): PersistSettings::list_mode
};

// `out_npix` = elements of the output images: W*H, or more when packed stripes overhang the frame (caller-owned gather
// buffers).  has_table: the launch walks the interior-descriptor table (else the records); has_cams: the frames of the batch
// carry their own cameras; have_spare: the build has the spare-ray kernel (then lim.max_per_cu_spare has been asked).
inline PersistPlan persist_plan(const PersistSettings &s, const PersistLimits &lim, const Frame &f, LaunchShape shape, int overlap_sets,
                                bool has_table, bool has_cams, bool have_spare, size_t out_npix,
                                unsigned long long fold_budget = kFoldBytes) {
  PersistPlan p;
  const int nb = f.batch > 1 ? f.batch : 1;
  p.spare = persist_uses_spare(s, has_table, have_spare);
  p.per_cu = persist_waves_per_cu(s, p.spare ? lim.max_per_cu_spare : (has_table ? lim.max_per_cu_desc : lim.max_per_cu), shape, overlap_sets);
  p.full_blocks = (lim.cus - s.cus_reserved) * p.per_cu;
  p.thresh_num = persist_thresh(s, p.spare);

  const int spp = f.spp < 1 ? 1 : f.spp;
  const bool resolve = spp > 1 || f.progressive;   // colours go through the float planes and a resolve kernel
  p.sequence = f.progressive && f.seq > 1;
  const int per_pixel = p.sequence ? f.seq : spp;
  if (persist_can_fold(f, per_pixel, fold_budget)) p.fold = per_pixel;
  p.invalid = p.sequence && (p.fold != f.seq || spp != 1);
  p.launches = p.fold > 1 ? 1 : spp;
  p.resolve = !resolve ? PersistPlan::kNone : (p.sequence ? PersistPlan::kSequence : (p.fold > 1 ? PersistPlan::kTiles : PersistPlan::kPlanes));
  p.npix = f.batch > 1 && (size_t)f.batch * (size_t)f.frame_stride > out_npix ? (size_t)f.batch * (size_t)f.frame_stride : out_npix;
  if (resolve) p.facc_floats = p.fold > 1 ? (size_t)(192ull * (unsigned long long)p.fold * (unsigned long long)f.ntiles * (unsigned long long)nb) : 3 * p.npix;

  // Consecutive frame numbers under one camera (the reference's still camera: frameNumber advances only while the camera stands,
  // Main.java:225-233) share their primary rays in mode 0: one slot per pixel, the primary cast once for the whole batch.  Frames
  // with their own cameras, several samples per pixel (folded or a launch each) / sequences, beam launches, paths of the primary
  // ray alone (every frame of those is the same image), the record walk and the spare-ray kernel keep a slot per (frame, pixel).
  p.span = s.span_mode != 0 && f.render_mode == 0 && !has_cams && p.fold == 1 && !resolve && f.batch > 1 && f.bounces >= 2 &&
           f.use_beam == 0 && has_table && !p.spare;
  p.slot_frames = p.span ? 1 : nb;
  p.rows_per_band = (f.tiles_y + 7) / 8;
  {
    const int last_rows = p.rows_per_band > 0 ? f.tiles_y % p.rows_per_band : 0;   // the one band that is not full (if any)
    const uint32_t tpf[2] = {(uint32_t)(p.rows_per_band * f.tiles_x * p.fold), (uint32_t)(last_rows * f.tiles_x * p.fold)};
    const uint64_t frames = (uint64_t)p.slot_frames;
    p.mg_rows[0] = udiv_magic((uint32_t)p.rows_per_band, (uint64_t)p.rows_per_band * (uint64_t)f.tiles_x);
    p.mg_rows[1] = udiv_magic((uint32_t)last_rows, (uint64_t)last_rows * (uint64_t)f.tiles_x);
    p.mg_tpf[0] = udiv_magic(tpf[0], frames * tpf[0]);   // n = slot >> 6 < frames x tile slots per frame
    p.mg_tpf[1] = udiv_magic(tpf[1], frames * tpf[1]);
  }
  const long long work = (long long)f.ntiles * p.slot_frames * p.fold;
  p.blocks = work < (long long)p.full_blocks ? (int)work : p.full_blocks;
  // (the records of all counter sets grow at once, for as many waves as a launch of this shape can have)
  if (p.span) p.prim_waves = (size_t)(p.full_blocks > p.blocks ? p.full_blocks : p.blocks);

  // the row / column tables: launches that carry one sample per pixel (samples / sequences folded into a launch seed every
  // sample of a pixel differently and keep computing in the round), on the descriptor walk, not the spare-ray kernel
  p.tables = s.table_mode != 0 && has_table && !p.spare && p.fold == 1;
  if (p.tables) {
    p.rc_stride = (size_t)((2 * f.width + 3) & ~3) + 8 * (size_t)f.height;
    p.rc_floats = p.rc_stride * (size_t)nb;
  }
  // the primary-hit cache: static-camera batches without hit records (those would need a fourth plane), on the tables' kernels
  p.cache = p.span && s.kept_mode != 0 && f.write_hits == 0 && p.tables;
  if (p.cache) p.kept_records = (size_t)f.tiles_y * 8 * (size_t)f.width;
  // (with lists: a launch whose cache indices or frames do not fit an entry's last word shades in its rounds, persist_kept_kernel<false>)
  p.list = s.list_mode != 0;
  p.dense = p.cache && s.dense_mode != 0 && f.bounces == 2 && (!p.list || ray_list_fits(p.kept_records, nb));
  p.list = p.list && p.dense;
  if (p.dense) p.ray_records = p.kept_records * (size_t)nb;
  return p;
}

}  // namespace svo
