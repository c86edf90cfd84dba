// svo_hip.hip -- C-ABI implementation of include/svo_hip.h (libsvohip.so).
// The reference-side interface each entry point replaces is cited in the header.
#include "../../include/svo_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// SVO_VARIANTS=0 (libsvohip.so, what a host loads): pipeline 1 -- persistent waves over the descriptor table, with the record
// walk for pools the table cannot state -- and pipeline 0 (the reference's one-thread-per-pixel decomposition: its kernel is also
// the counting pass of svo_count_frame), the beam pass, the builder, the ring, the group.
// SVO_VARIANTS=1 (libsvohip_variants.so, `make variants`; loaded by the tests that compare against them, like cxxloop): the same
// plus the comparators -- pipeline 2 (staged wavefront tracing), the spare-ray kernel of round 5 (SVO_SPARE=1) -- and the
// environment switches of the A/B runs (SVO_DERIVED, SVO_RC_TABLE, SVO_NORMAL_TABLE, SVO_BATCH_PRIMARY, SVO_FORCE_CAMS, SVO_PERSIST_*, ...).
#ifndef SVO_VARIANTS
#define SVO_VARIANTS 0
#endif
#include "svo_fused.hip.h"
#include "svo_persistent.hip.h"
#if SVO_ASM_LOOP && SVO_VARIANTS
#include "variants/svo_persist2.hip.h"
#endif
#if SVO_VARIANTS
#include "variants/svo_wavefront.hip.h"
#endif
#include "svo_build.hip.h"
#include "svo_beam.hip.h"
#include "svo_derive.hip.h"
#include "svo_brush.hip.h"
#include "svo_compact.hip.h"
#include "svo_rays.hip.h"

using namespace svo;

static_assert(sizeof(svo_hit) == 16, "svo_hit must be 16 bytes");

// The three output planes of a frame (or of a slot's frames): all allocated, or none (alloc_planes).
struct Planes { uint32_t *color = nullptr; float *depth = nullptr; uint4 *hits = nullptr; };

static void free_planes(Planes &p) {
  if (p.color) (void)hipFree(p.color);
  if (p.depth) (void)hipFree(p.depth);
  if (p.hits) (void)hipFree(p.hits);
  p = Planes();
}

// n_elems elements per plane, all planes or none: `out` is written only when every allocation succeeded
static hipError_t alloc_planes(size_t n_elems, bool want_hits, Planes &out) {
  Planes p;
  hipError_t e = hipMalloc((void **)&p.color, n_elems * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&p.depth, n_elems * 4);
  if (e == hipSuccess && want_hits) e = hipMalloc((void **)&p.hits, n_elems * 16);
  if (e == hipSuccess) out = p;
  else free_planes(p);
  return e;
}

// One {stream, images} set of the library's own (svo_dispatch_async takes turns on them)
struct ImageSet : Planes {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;   // behind the last overlapped dispatch into the set: a set is rendered into again only once that
  bool used = false;           // frame is complete -- at most `overlap` frames are queued
};

// svo_dispatch_async takes turns on `overlap` sets {stream, images} while the library owns them (the reference's loop, Main.java:132-146,
// 257-289: frame N + 1 starts in frame N's tail).  Set 0's stream is the context's own: made with it and kept for its lifetime, and
// its planes are the ones svo_resize makes.  The other sets' streams and planes, and every `done` event, are made on first use
// (take_next); the planes go with every svo_resize (free_images), the streams and events with the context (free_state).
// The context's stream / d_* always name ONE set, the one of the last dispatch, so every read-back sees the last dispatched frame.
struct ImageSets {
  static constexpr int kMax = 8;
  ImageSet set[kMax];
  int cur = 0;
  int overlap = 4;                // sets svo_dispatch_async takes turns on (svo_set_overlap; 1 = no alternation)
  bool others_inflight = false;   // a set that is not current may still have a frame in flight
  ImageSet &operator[](int i) { return set[i]; }
  ImageSet &current() { return set[cur]; }
  bool is_own_stream(hipStream_t st) const {
    for (const ImageSet &s : set) if (s.stream && st == s.stream) return true;
    return false;
  }
  // waits for the frames in flight on every set's stream
  hipError_t sync_own_streams() {
    for (ImageSet &s : set)
      if (s.stream) { const hipError_t e = hipStreamSynchronize(s.stream); if (e != hipSuccess) return e; }
    others_inflight = false;
    return hipSuccess;
  }
  // The next set in turn, for a frame of n pixels, made whole before it is named: its stream, its zeroed planes, its event, and its
  // previous frame complete -- the host runs ahead of the GPU by at most `overlap` frames (a swap chain's depth; the pick launches
  // do not throttle it any more: they need a wave slot, not the frame's turn).  A failed step leaves `cur` as it was, and the next
  // call tries again.
  hipError_t take_next(size_t n) {
    const int k = (cur + 1) % overlap;
    ImageSet &s = set[k];
    hipError_t e;
    if (!s.stream && (e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess) return e;
    if (!s.color) {
      if ((e = alloc_planes(n, true, s)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(s.color, 0, n * 4, s.stream)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(s.depth, 0, n * 4, s.stream)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(s.hits, 0, n * 16, s.stream)) != hipSuccess) return e;
    }
    if (!s.done && (e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return e;
    if (s.used && (e = hipEventSynchronize(s.done)) != hipSuccess) return e;
    cur = k;
    others_inflight = true;
    return hipSuccess;
  }
  // the image size ends: every set's planes go and set 0 is current again; `stream` (the context's) follows if it named a set
  void free_images(hipStream_t &stream) {
    for (ImageSet &s : set) { free_planes(s); s.used = false; }
    if (cur != 0 && (is_own_stream(stream) || stream == nullptr)) stream = set[0].stream;
    cur = 0; others_inflight = false;
  }
  // the context ends (behind free_images)
  void free_state() {
    for (ImageSet &s : set) {
      if (s.done) (void)hipEventDestroy(s.done);
      if (s.stream) (void)hipStreamDestroy(s.stream);
      s = ImageSet();
    }
  }
};

#include "svo_ring.hip.h"   // RingSlot, Ring (its functions: further down)

// What a context keeps, by the three lifetimes its state has.  Each lifetime ends in ONE function below, which has one line per
// feature, all three in the same order (beam, pick, sets, ring, persist, derive, brush, compact, rays):
//   the context         svo_destroy     beam::State (events, live table), pick::State, ImageSets (streams, events), Ring::reserved_cus,
//                                       PersistSettings / PersistLimits, derive::Table, brush::State, compact::State, rays::State
//   the image size      free_outputs    beam::State (images), pick::State::live, ImageSets (planes), Ring (the slots), PersistBuffers
//                       (svo_resize)    [+ WavefrontBuffers in a variants build]
//   the pool's contents pool_changed    beam::State::live_valid, derived_valid, PersistSettings::pool_epoch + the primary-hit cache's key
// A feature that gains a buffer puts it into its own struct and frees it in that struct's function for the lifetime; a new feature
// adds its line to the functions whose lifetimes it has.
struct svo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;       // the stream dispatches go to: the current set's, or the caller's (svo_set_stream)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // pool
  uint8_t *d_pool = nullptr;
  uint64_t pool_len = 0, pool_cap = 0;
  uint32_t dword0 = 0;
  // frame state
  float cam[15] = {1.5f, 1.5f, 2.0f, -1.6f, -0.9f, -1.f, -1.6f, 0.9f, -1.f, 1.6f, -0.9f, -1.f, 1.6f, 0.9f, -1.f};
  int width = 0, height = 0, y0 = 0, y1 = 0;
  bool rows_set = false;
  int row_step = 1, out_y0 = 0, n_tile_rows = -1;  // stripe mode (svo_set_stripes); n_tile_rows < 0 = band mode
  int frame_number = 2, render_mode = 2, buffer_end = 0, use_beam = 0, bounces = 2, spp = 1, progressive = 0;
  int seq = 1, seq_fresh = 0;    // progressive: frames of the accumulation per dispatch, on a zeroed image or not (svo_set_sequence)
  int batch = 1;                 // frames per dispatch (svo_set_batch)
  uint64_t frame_stride = 0;     // elements between consecutive frames of a batch in each output
  uint32_t mirror_mask = 0;
  int pipeline = 1;        // persistent waves on the descriptor table; 0 / 2: svo_set_pipeline
  int write_hits = 1;
  // outputs
  uint32_t *d_color = nullptr;
  float *d_depth = nullptr;
  uint4 *d_hits = nullptr;
  bool external_outputs = false;
  DeviceCounters *d_counters = nullptr;
  float4 *d_ntab = nullptr;   // unit normal of every 16-bit normal code (svo_trav2.h::normal_table_kernel), made with the context
  // the features' state, in the order of the lifetime functions
  beam::State beam;           // the beam pre-pass: images, their events, the live-node table of the pool (svo_beam.hip.h)
  pick::State pick;           // the pick pixel (svo_set_pick): answered from pinned host memory a one-wave launch writes (svo_fused.hip.h)
  ImageSets sets;             // the {stream, images} sets of svo_dispatch_async
  Ring ring;                  // frames in flight behind the boundary (svo_ring_*, svo_ring.hip.h)
  PersistState pb;            // the persistent pipeline: settings (they outlive svo_resize), device limits, per-size buffers
#if SVO_VARIANTS
  WavefrontBuffers wf;
#endif
  // interior-descriptor table of the pool (svo_derive.hip.h): rebuilt lazily after every pool change, walked by the
  // persistent pipeline when the pool is derivable
  derive::Table dt;
  bool derived_valid = false;     // cleared by everything that changes the pool
  int derived_mode = 1;           // 0 = always walk the records, 1 = walk the table when there is one
  brush::State bs;             // work items and counters of svo_brush_* (made at the first stroke), what the last stroke did
  compact::State cs;           // events of svo_pool_compact (made at the first call), what the last call did
  rays::State rs;              // counters, staging buffers and counts of svo_cast_rays* (made at the first call)
  std::vector<void *> ipc_opened;
  std::vector<void *> dev_allocs;   // svo_dev_alloc, freed with the context at the latest
  svo_stats stats{};
  std::string err;
};

static int fail(svo_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return fail(ctx, SVO_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));            \
  } while (0)

static constexpr uint64_t kPad = 64;  // zero bytes kept behind the pool (8-byte record loads may overhang)

// Where one launch goes and which frames it renders.  make_frame, launch_frame, launch_frame_kernels and launch_pick
// read these from here and everything else (render mode, bounces, spp, rows and stripes, pipeline, ...) from the context.
struct Target {
  hipStream_t stream = nullptr;
  Planes out;
  bool external = false;         // the planes are the caller's (svo_bind_outputs, svo_ring_bind_slot, a ring slot's frame range)
  int batch = 1;                 // frames of the launch, frame_stride elements apart in each plane
  uint64_t frame_stride = 0;
  int frame_number = 0;
  float cam[15] = {};
  const FrameVar *cams = nullptr;         // per-frame cameras / frame numbers of the batch (svo_ring_submit_cams), on the host, ...
  RingSlot *cams_slot = nullptr;          // ... and the slot that keeps them on the device (d_fvar) and stages the copy (ring_copy_cams)
  LaunchShape shape = kPlain;                              // the persistent launch's shape unless svo_set_tuning named one
  int overlap_sets = 0;                                    // kOverlap: the number of sets taking turns
};

// the context's own dispatch state: the set of the last dispatch (or the caller's stream and outputs), its camera and frame number
static Target current_target(const svo_ctx *c) {
  Target t;
  t.stream = c->stream; t.out = {c->d_color, c->d_depth, c->d_hits}; t.external = c->external_outputs;
  t.batch = c->batch; t.frame_stride = c->frame_stride; t.frame_number = c->frame_number;
  memcpy(t.cam, c->cam, sizeof t.cam);
  return t;
}

// The pool's contents end.  Every pool mutator starts here, before its argument checks: the pool is about to change (or to be
// handed out for writing), so what was derived from it no longer describes it.  (pick, sets, ring, brush, compact and rays keep
// nothing that describes the pool.)
static void pool_changed(svo_ctx *c) {
  if (!c) return;
  beam::pool_changed(c->beam);      // the live-node table
  persist_pool_changed(c->pb);      // the primary-hit cache: part of its key, and empty from here on
  c->derived_valid = false;         // the descriptor table: rebuilt (or refreshed, svo_pool_update) before the next cast
}

static void ring_free(svo_ctx *c);   // svo_ring.hip.h

// The image size ends (svo_resize; the context's end goes through here first).  The device is idle.  (derive, brush, compact and
// rays keep nothing of the image's size.)
static void free_outputs(svo_ctx *c) {
  beam::free_images(c->beam);
  c->pick.invalidate();
  c->sets.free_images(c->stream);   // (the streams and the events stay)
  ring_free(c);                     // the ring's images have the size of the frame
  persist_free(c->pb.buf);
#if SVO_VARIANTS
  wavefront_free(c->wf);
#endif
  if (!c->external_outputs) { c->d_color = nullptr; c->d_depth = nullptr; c->d_hits = nullptr; }
}

extern "C" {

int svo_create(int device, svo_ctx **out) {
  if (!out) return SVO_E_INVALID;
  *out = nullptr;
  // Frames in flight (svo_ring_*) want a hardware queue per stream; HIP maps streams onto GPU_MAX_HW_QUEUES queues
  // (default 4: two frame streams on one queue serialise their launches).  Read when the runtime starts, so this only
  // has an effect when the library makes the process's first HIP call (a JVM host); it never overrides the caller's value.
  (void)setenv("GPU_MAX_HW_QUEUES", "8", 0);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SVO_E_NODEVICE;
  svo_ctx *c = new svo_ctx();
  c->device = device;
  c->stats.device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->sets[0].stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipMalloc((void **)&c->d_counters, sizeof(DeviceCounters)) != hipSuccess) {
    delete c;
    return SVO_E_HIP;
  }
  c->stream = c->sets[0].stream;
  // the normal table: 65 536 x 16 bytes, a function of nothing but the code
  if (hipMalloc((void **)&c->d_ntab, 65536 * sizeof(float4)) == hipSuccess) {
    hipLaunchKernelGGL(normal_table_kernel, dim3(256), dim3(256), 0, c->sets[0].stream, c->d_ntab);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->sets[0].stream) != hipSuccess) { (void)hipFree(c->d_ntab); c->d_ntab = nullptr; }
  }
  *out = c;
  return SVO_OK;
}

// The context ends: what free_outputs leaves of every feature, then what belongs to no feature.
int svo_destroy(svo_ctx *c) {
  if (!c) return SVO_E_INVALID;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  free_outputs(c);
  beam::free_state(c->beam);
  pick::free_state(c->pick);
  c->sets.free_state();
  // (ring, persist: settings and counts only, nothing to free)
  derive::free_table(c->dt);
  brush::free_state(c->bs);
  compact::free_state(c->cs);
  rays::free_state(c->rs);
  if (c->d_pool) (void)hipFree(c->d_pool);
  if (c->d_counters) (void)hipFree(c->d_counters);
  if (c->d_ntab) (void)hipFree(c->d_ntab);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  for (void *p : c->ipc_opened) if (p) (void)hipIpcCloseMemHandle(p);
  for (void *p : c->dev_allocs) if (p) (void)hipFree(p);
  delete c;
  return SVO_OK;
}

const char *svo_last_error(const svo_ctx *c) { return c ? c->err.c_str() : "null context"; }

int svo_build_info(void) { return (SVO_VARIANTS ? 1 : 0) | (SVO_ASM_LOOP ? 2 : 0); }

// ---------------------------------------------------------------- pool
static int ensure_pool_capacity(svo_ctx *c, uint64_t need_len, bool keep) {
  if (need_len >= 0x80000000ull) return fail(c, SVO_E_TOOLARGE, "pool must stay below 2^31 bytes");
  const uint64_t need = need_len + kPad;
  if (need <= c->pool_cap) return SVO_OK;
  uint64_t ncap = keep ? std::max<uint64_t>(need, c->pool_cap + c->pool_cap / 4) : need;
  uint8_t *np = nullptr;
  HIPCHK(c, hipMalloc((void **)&np, ncap));
  HIPCHK(c, hipMemsetAsync(np, 0, ncap, c->sets[0].stream));
  if (keep && c->d_pool && c->pool_len)
    HIPCHK(c, hipMemcpyAsync(np, c->d_pool, c->pool_len, hipMemcpyDeviceToDevice, c->sets[0].stream));
  HIPCHK(c, hipStreamSynchronize(c->sets[0].stream));
  if (c->d_pool) HIPCHK(c, hipFree(c->d_pool));   // callers have synchronised the device: no frame still reads it
  c->d_pool = np;
  c->pool_cap = ncap;
  return SVO_OK;
}

static int refresh_dword0(svo_ctx *c) {
  c->dword0 = 0;
  if (c->pool_len >= 4) HIPCHK(c, hipMemcpy(&c->dword0, c->d_pool, 4, hipMemcpyDeviceToHost));
  else if (c->pool_len > 0) HIPCHK(c, hipMemcpy(&c->dword0, c->d_pool, c->pool_len, hipMemcpyDeviceToHost));
  return SVO_OK;
}

int svo_pool_reserve(svo_ctx *c, uint64_t nbytes) {
  pool_changed(c);
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  int rc = ensure_pool_capacity(c, nbytes, false);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_pool, 0, c->pool_cap, c->sets[0].stream));
  HIPCHK(c, hipStreamSynchronize(c->sets[0].stream));
  c->pool_len = nbytes;
  return SVO_OK;
}

int svo_pool_upload_device(svo_ctx *c, const void *dptr, uint64_t nbytes) {
  pool_changed(c);
  if (!c || (!dptr && nbytes)) return fail(c, SVO_E_INVALID, "svo_pool_upload_device: null buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  int rc = ensure_pool_capacity(c, nbytes, false);
  if (rc) return rc;
  if (nbytes) HIPCHK(c, hipMemcpy(c->d_pool, dptr, nbytes, hipMemcpyDeviceToDevice));
  HIPCHK(c, hipMemset(c->d_pool + nbytes, 0, c->pool_cap - nbytes));
  c->pool_len = nbytes;
  return refresh_dword0(c);
}

int svo_pool_upload(svo_ctx *c, const void *host, uint64_t nbytes) {
  pool_changed(c);
  if (!c || (!host && nbytes)) return fail(c, SVO_E_INVALID, "svo_pool_upload: null buffer");
  HIPCHK(c, hipSetDevice(c->device));
  // frames may be in flight on any stream the caller has handed over (svo_set_stream): the pool changes only
  // when the whole device is idle, so a frame sees either the old bytes or the new ones, never a mix
  HIPCHK(c, hipDeviceSynchronize());
  int rc = ensure_pool_capacity(c, nbytes, false);
  if (rc) return rc;
  if (nbytes) HIPCHK(c, hipMemcpy(c->d_pool, host, nbytes, hipMemcpyHostToDevice));
  // bytes behind the new end must read as zero
  HIPCHK(c, hipMemset(c->d_pool + nbytes, 0, c->pool_cap - nbytes));
  c->pool_len = nbytes;
  return refresh_dword0(c);
}

int svo_pool_update(svo_ctx *c, const void *host_base, uint64_t start, uint64_t end) {
  // a walkable descriptor table follows a ranged update instead of being rebuilt (derive::refresh_table): an SDF brush
  // stroke is two such updates (Main.java:349-350), the table of the 8192^3 scene takes 6.7 ms to build
#if SVO_VARIANTS
  static const bool follow = []() { const char *e = getenv("SVO_DERIVED_REFRESH"); return !(e && e[0] == '0'); }();
#else
  const bool follow = true;
#endif
  const bool had_table = c && follow && c->derived_valid && c->dt.ok;
  pool_changed(c);
  if (!c || !host_base) return fail(c, SVO_E_INVALID, "svo_pool_update: null buffer");
  if (start >= end) return fail(c, SVO_E_INVALID, "Update SSBO error: Invalid parameters.");
  if (!c->d_pool) return fail(c, SVO_E_NOPOOL, "svo_pool_update before svo_pool_upload");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());   // see svo_pool_upload
  if (end > c->pool_len) {
    int rc = ensure_pool_capacity(c, end, true);
    if (rc) return rc;
  }
  HIPCHK(c, hipMemcpy(c->d_pool + start, (const uint8_t *)host_base + start, end - start, hipMemcpyHostToDevice));
  if (end > c->pool_len) c->pool_len = end;
  if (start < 4) { int rc = refresh_dword0(c); if (rc) return rc; }
  if (had_table) {
    bool refreshed = false;
    hipError_t e = derive::refresh_table(c->dt, c->d_pool, c->pool_len, start, end, c->sets[0].stream, &refreshed);
    if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string("descriptor table refresh: ") + hipGetErrorString(e));
    c->derived_valid = refreshed;   // false: the next dispatch builds it anew
  }
  return SVO_OK;
}

int svo_pool_download(svo_ctx *c, void *host, uint64_t nbytes) {
  if (!c || !host) return fail(c, SVO_E_INVALID, "svo_pool_download: null buffer");
  if (!c->d_pool) return fail(c, SVO_E_NOPOOL, "no pool");
  if (nbytes > c->pool_len) nbytes = c->pool_len;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(host, c->d_pool, nbytes, hipMemcpyDeviceToHost));
  return SVO_OK;
}

int svo_pool_device_ptr(svo_ctx *c, void **dptr, uint64_t *nbytes) {
  pool_changed(c);
  if (!c || !dptr) return SVO_E_INVALID;
  *dptr = c->d_pool;
  if (nbytes) *nbytes = c->pool_len;
  // the caller may have written the pool through this pointer (RCCL broadcast): re-read dword 0
  if (c->d_pool) {
    HIPCHK(c, hipSetDevice(c->device));
    return refresh_dword0(c);
  }
  return SVO_OK;
}

int svo_pool_commit(svo_ctx *c) {
  pool_changed(c);
  if (!c) return SVO_E_INVALID;
  if (!c->d_pool) return fail(c, SVO_E_NOPOOL, "svo_pool_commit: no pool");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());   // the caller's writes (any stream) and every frame in flight
  return refresh_dword0(c);
}

int svo_pool_download_range(svo_ctx *c, void *host_base, uint64_t start, uint64_t end) {
  if (!c || !host_base) return fail(c, SVO_E_INVALID, "svo_pool_download_range: null buffer");
  if (!c->d_pool) return fail(c, SVO_E_NOPOOL, "no pool");
  if (start >= end || end > c->pool_len) return fail(c, SVO_E_INVALID, "svo_pool_download_range: need start < end <= the pool's length");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy((uint8_t *)host_base + start, c->d_pool + start, end - start, hipMemcpyDeviceToHost));
  return SVO_OK;
}

// ---------------------------------------------------------------- SDF brush (svo_brush.hip.h)
// Main.placeSDF (Main.java:338-353) without the host: plan on the device, grow the pool once, write, let the table follow
static int brush_stroke(svo_ctx *c, const brush::Sdf &s, int value, int world_size, int max_lod, int32_t cb[4], const char *who) {
  if (world_size == 0) world_size = 8196;   // Constants.WORLD_SIZE (sic)
  if (max_lod == 0) max_lod = 13;
  if (value < 0 || value > 255) return fail(c, SVO_E_INVALID, std::string(who) + ": value must be a byte (0..255)");
  if (world_size < 1 || world_size > brush::kMaxWorld || max_lod < 1 || max_lod > 15)
    return fail(c, SVO_E_INVALID, std::string(who) + ": world_size 1..32768 and max_lod 1..15");
  for (int i = 0; i < 3; i++)
    if (s.o[i] < -(1 << 20) || s.o[i] > (1 << 20)) return fail(c, SVO_E_INVALID, std::string(who) + ": origin out of range");
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, std::string(who) + ": no pool uploaded");
  const bool had_table = c->derived_valid && c->dt.ok;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());   // see svo_pool_upload
  hipStream_t st = c->sets[0].stream;
  brush::State &b = c->bs;
  if (!b.ctr) HIPCHK(c, hipMalloc((void **)&b.ctr, brush::kCtrWords * sizeof(uint32_t)));
  if (!b.e0) HIPCHK(c, hipEventCreate(&b.e0));
  if (!b.e1) HIPCHK(c, hipEventCreate(&b.e1));
  const uint32_t start1 = (uint32_t)c->pool_len;
  HIPCHK(c, hipEventRecord(b.e0, st));
  brush::Plan p;
  for (;;) {
    if (!b.items) {
      if (!b.cap) b.cap = brush::kFirstCap;
      hipError_t e = hipMalloc((void **)&b.items, (size_t)b.cap * sizeof(brush::Item));
      if (e != hipSuccess) { b.items = nullptr; b.cap = 0; return fail(c, SVO_E_HIP, std::string(who) + ": work items: " + hipGetErrorString(e)); }
    }
    p = brush::Plan();
    hipError_t e = brush::plan(b, c->d_pool, start1, s, value, world_size, max_lod, st, p);
    if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    if (!(p.flags & brush::kFlagItems)) break;
    if (b.cap >= brush::kLastCap) return fail(c, SVO_E_TOOLARGE, std::string(who) + ": the stroke visits more nodes than the work lists hold");
    HIPCHK(c, hipFree(b.items));   // the plan wrote nothing but its items: again, with four times the room
    b.items = nullptr;
    b.cap *= 4;
  }
  if (p.flags & brush::kFlagBounds) return fail(c, SVO_E_INVALID, std::string(who) + ": a record the stroke reaches lies outside the pool");
  if (p.flags & brush::kFlagShortLeaf)
    return fail(c, SVO_E_INVALID, std::string(who) + ": the stroke would subdivide a 3-byte or 1-byte leaf (max_lod does not match the tree)");
  const uint64_t new_len = (uint64_t)start1 + p.appended;
  int rc = ensure_pool_capacity(c, new_len, true);   // SVO_E_TOOLARGE from 2^31 bytes on; the pool as it was
  if (rc) return rc;
  // from here on the pool changes
  pool_changed(c);
  hipLaunchKernelGGL(brush::write_kernel, dim3((p.items + 255u) / 256u), dim3(256), 0, st, c->d_pool, start1, b.items, p.items, value, b.ctr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(b.e1, st));
  uint32_t h[brush::kCtrWords];
  HIPCHK(c, hipMemcpyAsync(h, b.ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->pool_len = new_len;
  const uint32_t lo = h[brush::kCtrHi] ? h[brush::kCtrLo] : 0u, hi = h[brush::kCtrHi];
  if (cb) { cb[0] = (int32_t)h[brush::kCtrStart0]; cb[1] = (int32_t)h[brush::kCtrEnd0]; cb[2] = (int32_t)start1; cb[3] = (int32_t)new_len; }
  b.strokes++; b.visited = p.items; b.subdivided = h[brush::kCtrSubdivided]; b.lo = lo; b.hi = hi;
  (void)hipEventElapsedTime(&b.gpu_ms, b.e0, b.e1);
  if (hi > lo && lo < 4) { rc = refresh_dword0(c); if (rc) return rc; }
  if (had_table) {
    // what the two svo_pool_update calls of the host route do: the table follows [lo, hi) and [start1, end1)
    bool refreshed = true;
    const uint64_t ranges[2][2] = {{lo, hi}, {start1, new_len}};
    for (int k = 0; k < 2 && refreshed; k++) {
      if (ranges[k][0] >= ranges[k][1]) continue;
      hipError_t e = derive::refresh_table(c->dt, c->d_pool, c->pool_len, ranges[k][0], ranges[k][1], st, &refreshed);
      if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string("descriptor table refresh: ") + hipGetErrorString(e));
    }
    c->derived_valid = refreshed;   // false: the next dispatch builds it anew
  }
  return SVO_OK;
}

int svo_brush_sphere(svo_ctx *c, const int origin[3], int radius, int value, int world_size, int max_lod, int32_t cb[4]) {
  if (!c || !origin) return fail(c, SVO_E_INVALID, "svo_brush_sphere: null origin");
  if (radius < 0 || radius > (1 << 20)) return fail(c, SVO_E_INVALID, "svo_brush_sphere: radius out of range");
  brush::Sdf s{};
  s.kind = 0; s.r = radius;
  for (int i = 0; i < 3; i++) { s.o[i] = origin[i]; s.mn[i] = origin[i] - radius - 1; s.mx[i] = origin[i] + radius + 1; }   // Sphere.java
  return brush_stroke(c, s, value, world_size, max_lod, cb, "svo_brush_sphere");
}

int svo_brush_box(svo_ctx *c, const int origin[3], int w, int h, int d, int value, int world_size, int max_lod, int32_t cb[4]) {
  if (!c || !origin) return fail(c, SVO_E_INVALID, "svo_brush_box: null origin");
  const int ext[3] = {w, h, d};
  brush::Sdf s{};
  s.kind = 1;
  for (int i = 0; i < 3; i++) {
    if (ext[i] < 0 || ext[i] > (1 << 20)) return fail(c, SVO_E_INVALID, "svo_brush_box: extent out of range");
    const int half = (ext[i] + 1) / 2;   // (int)Math.ceil(w / 2.0f), Box.java
    s.o[i] = origin[i]; s.b[i] = ext[i]; s.mn[i] = origin[i] - half; s.mx[i] = origin[i] + half;
  }
  return brush_stroke(c, s, value, world_size, max_lod, cb, "svo_brush_box");
}

int svo_brush_info(svo_ctx *c, uint64_t *strokes, uint64_t *visited, uint64_t *subdivided, uint64_t *lo, uint64_t *hi, float *gpu_ms) {
  if (!c) return SVO_E_INVALID;
  if (strokes) *strokes = c->bs.strokes;
  if (visited) *visited = c->bs.visited;
  if (subdivided) *subdivided = c->bs.subdivided;
  if (lo) *lo = c->bs.lo;
  if (hi) *hi = c->bs.hi;
  if (gpu_ms) *gpu_ms = c->bs.gpu_ms;
  return SVO_OK;
}

// ---------------------------------------------------------------- compaction (svo_compact.hip.h)
int svo_pool_compact(svo_ctx *c, uint64_t *old_nbytes, uint64_t *new_nbytes) {
  if (!c) return SVO_E_INVALID;
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, "svo_pool_compact: no pool uploaded");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());   // see svo_pool_upload
  hipStream_t st = c->sets[0].stream;
  compact::State &s = c->cs;
  if (!s.e0) HIPCHK(c, hipEventCreate(&s.e0));
  if (!s.e1) HIPCHK(c, hipEventCreate(&s.e1));
  HIPCHK(c, hipEventRecord(s.e0, st));
  compact::Result r;
  hipError_t e = compact::run(c->d_pool, (uint32_t)c->pool_len, kPad, st, r);
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string("svo_pool_compact: ") + hipGetErrorString(e));
  if (old_nbytes) *old_nbytes = c->pool_len;
  if (new_nbytes) *new_nbytes = r.refusal == compact::kTooLarge ? r.len : c->pool_len;
  switch (r.refusal) {
    case compact::kOutside: return fail(c, SVO_E_INVALID, "svo_pool_compact: a children block the tree reaches lies outside the pool");
    case compact::kTooDeep: return fail(c, SVO_E_INVALID, "svo_pool_compact: the tree has more levels than the walk supports (or a cycle)");
    case compact::kTooManyNodes: return fail(c, SVO_E_TOOLARGE, "svo_pool_compact: more reachable nodes than the node lists may hold");
    case compact::kTooLarge: return fail(c, SVO_E_TOOLARGE, "pool must stay below 2^31 bytes");
    case compact::kDone: break;
  }
  HIPCHK(c, hipEventRecord(s.e1, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // from here on the pool changes
  pool_changed(c);
  (void)hipFree(c->d_pool);
  c->d_pool = r.pool; c->pool_len = r.len; c->pool_cap = r.cap;
  if (new_nbytes) *new_nbytes = r.len;
  s.calls++; s.records = 1u + 8u * r.nodes; s.levels = r.levels;
  (void)hipEventElapsedTime(&s.gpu_ms, s.e0, s.e1);
  return refresh_dword0(c);
}

int svo_compact_info(svo_ctx *c, uint64_t *calls, uint64_t *records, int *levels, float *gpu_ms) {
  if (!c) return SVO_E_INVALID;
  if (calls) *calls = c->cs.calls;
  if (records) *records = c->cs.records;
  if (levels) *levels = c->cs.levels;
  if (gpu_ms) *gpu_ms = c->cs.gpu_ms;
  return SVO_OK;
}

// ---------------------------------------------------------------- world generation
__global__ void count_zero_bytes_kernel(const uint8_t *p, size_t n, unsigned int *zeros) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int z = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) z += p[i] == 0 ? 1u : 0u;
  if (z) atomicAdd(zeros, z);
}

// the tail of both builders: `e` is what the build returned; a pool that fits replaces the context's
static int adopt_built_pool(svo_ctx *c, hipError_t e, const build::Result &r, bool too_large, uint64_t *out_nbytes, const char *who) {
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (out_nbytes) *out_nbytes = r.len;
  if (too_large) return fail(c, SVO_E_TOOLARGE, "pool must stay below 2^31 bytes");
  if (c->d_pool) (void)hipFree(c->d_pool);
  c->d_pool = r.pool; c->pool_len = r.len; c->pool_cap = r.cap;
  return refresh_dword0(c);
}

int svo_build_from_heightmap(svo_ctx *c, const uint16_t *height, const uint8_t *material, int n, uint64_t *out_nbytes) {
  pool_changed(c);
  if (!c || !height || !material) return fail(c, SVO_E_INVALID, "svo_build_from_heightmap: null map");
  if (n < 8 || n > 8192 || (n & (n - 1))) return fail(c, SVO_E_INVALID, "svo_build_from_heightmap: n must be a power of two in 8..8192");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const size_t cells = (size_t)n * (size_t)n;
  uint16_t *d_h = nullptr;
  uint8_t *d_m = nullptr;
  unsigned int *d_z = nullptr;
  auto cleanup = [&]() { if (d_h) (void)hipFree(d_h); if (d_m) (void)hipFree(d_m); if (d_z) (void)hipFree(d_z); };
  hipError_t e = hipMalloc((void **)&d_h, cells * 2);
  if (e == hipSuccess) e = hipMalloc((void **)&d_m, cells);
  if (e == hipSuccess) e = hipMalloc((void **)&d_z, 4);
  if (e == hipSuccess) e = hipMemcpyAsync(d_h, height, cells * 2, hipMemcpyHostToDevice, c->sets[0].stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_m, material, cells, hipMemcpyHostToDevice, c->sets[0].stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_z, 0, 4, c->sets[0].stream);
  unsigned int zeros = 0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(count_zero_bytes_kernel, dim3(1024), dim3(256), 0, c->sets[0].stream, d_m, cells, d_z);
    e = hipMemcpyAsync(&zeros, d_z, 4, hipMemcpyDeviceToHost, c->sets[0].stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->sets[0].stream);
  if (e != hipSuccess) { cleanup(); return fail(c, SVO_E_HIP, std::string("svo_build_from_heightmap: ") + hipGetErrorString(e)); }
  if (zeros) { cleanup(); return fail(c, SVO_E_INVALID, "svo_build_from_heightmap: material 0 in the material map (0 is the empty voxel)"); }
  build::Result r;
  bool too_large = false;
  e = build::build_pool(d_h, d_m, n, kPad, c->sets[0].stream, r, &too_large);
  cleanup();
  return adopt_built_pool(c, e, r, too_large, out_nbytes, "svo_build_from_heightmap");
}

int svo_build_from_heightmap16(svo_ctx *c, const uint16_t *raw16, const uint8_t *material, int n, uint64_t *out_nbytes) {
  if (!c || !raw16 || !material) return fail(c, SVO_E_INVALID, "svo_build_from_heightmap16: null map");
  if (n < 8 || n > 8192 || (n & (n - 1))) return fail(c, SVO_E_INVALID, "svo_build_from_heightmap16: n must be a power of two in 8..8192");
  // chunkgen-heightmap.comp:16-19: heightSample = int(r / 65536.0 * 2048) -- exact in float (two powers of two): r >> 5
  std::vector<uint16_t> h((size_t)n * (size_t)n);
  for (size_t i = 0; i < h.size(); i++) h[i] = (uint16_t)(raw16[i] >> 5);
  return svo_build_from_heightmap(c, h.data(), material, n, out_nbytes);
}

int svo_build_from_voxels(svo_ctx *c, const uint8_t *voxels, int n, uint64_t *out_nbytes) {
  pool_changed(c);
  if (!c || !voxels) return fail(c, SVO_E_INVALID, "svo_build_from_voxels: null grid");
  if (n < 2 || n > 1024 || (n & (n - 1))) return fail(c, SVO_E_INVALID, "svo_build_from_voxels: n must be a power of two in 2..1024");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const size_t cells = (size_t)n * (size_t)n * (size_t)n;
  uint8_t *d_v = nullptr;
  hipError_t e = hipMalloc((void **)&d_v, cells);
  if (e == hipSuccess) e = hipMemcpyAsync(d_v, voxels, cells, hipMemcpyHostToDevice, c->sets[0].stream);
  build::Result r;
  bool too_large = false;
  if (e == hipSuccess) e = build::build_pool_from_voxels(d_v, n, kPad, c->sets[0].stream, r, &too_large);
  if (d_v) (void)hipFree(d_v);
  return adopt_built_pool(c, e, r, too_large, out_nbytes, "svo_build_from_voxels");
}

// ---------------------------------------------------------------- frame state
int svo_set_camera(svo_ctx *c, const float pos[3], const float l1[3], const float l2[3], const float r1[3],
                   const float r2[3]) {
  if (!c || !pos || !l1 || !l2 || !r1 || !r2) return fail(c, SVO_E_INVALID, "svo_set_camera: null vector");
  memcpy(c->cam + 0, pos, 12); memcpy(c->cam + 3, l1, 12); memcpy(c->cam + 6, l2, 12);
  memcpy(c->cam + 9, r1, 12); memcpy(c->cam + 12, r2, 12);
  return SVO_OK;
}

int svo_set_params(svo_ctx *c, int frame_number, int render_mode, int buffer_end, int use_beam, int bounces,
                   uint32_t mirror_mask, int spp) {
  if (!c) return SVO_E_INVALID;
  if (bounces < 1 || spp < 1) return fail(c, SVO_E_INVALID, "bounces and spp must be >= 1");
  c->frame_number = frame_number; c->render_mode = render_mode; c->buffer_end = buffer_end; c->use_beam = use_beam;
  c->bounces = bounces; c->mirror_mask = mirror_mask; c->spp = spp;
  return SVO_OK;
}

int svo_resize(svo_ctx *c, int width, int height) {
  if (!c || width <= 0 || height <= 0) return fail(c, SVO_E_INVALID, "svo_resize: bad size");
  HIPCHK(c, hipSetDevice(c->device));
  ImageSet &own = c->sets[0];
  if (width == c->width && height == c->height && own.color) return SVO_OK;
  HIPCHK(c, hipDeviceSynchronize());   // frames in flight on other streams still write the old images
  free_outputs(c);
  const size_t n = (size_t)width * (size_t)height;
  HIPCHK(c, alloc_planes(n, true, own));
  HIPCHK(c, hipMemset(own.color, 0, n * 4));
  HIPCHK(c, hipMemset(own.depth, 0, n * 4));
  HIPCHK(c, hipMemset(own.hits, 0, n * 16));
  // hipMemset is asynchronous and the dispatch streams do not synchronise with the null stream: without this wait the
  // zeroing can land after the first frame's stores (seen as all-zero hit records of sky pixels)
  HIPCHK(c, hipDeviceSynchronize());
  if (!c->external_outputs) { c->d_color = own.color; c->d_depth = own.depth; c->d_hits = own.hits; }
  c->width = width; c->height = height;
  if (c->pick.follow_centre) { c->pick.x = width / 2; c->pick.y = height / 2; }   // the crosshair: Main.java:139-141 reads (WIDTH / 2, HEIGHT / 2)
  else if (c->pick.x >= width || c->pick.y >= height) { c->pick.x = -1; c->pick.y = -1; }
  c->y0 = 0; c->y1 = height; c->rows_set = false;  // a new image size resets the row band to the whole frame
  c->row_step = 1; c->out_y0 = 0; c->n_tile_rows = -1;
  return SVO_OK;
}

int svo_bind_outputs(svo_ctx *c, void *color, void *depth, void *hits) {
  if (!c) return SVO_E_INVALID;
  c->pick.invalidate();
  if (!color) {
    c->external_outputs = false;
    const ImageSet &s = c->sets.current();   // (a set is current only once it has its planes)
    c->d_color = s.color; c->d_depth = s.depth; c->d_hits = s.hits;
    return SVO_OK;
  }
  if (!depth) return fail(c, SVO_E_INVALID, "svo_bind_outputs: depth buffer required");
  c->external_outputs = true;
  c->d_color = (uint32_t *)color; c->d_depth = (float *)depth; c->d_hits = (uint4 *)hits;
  return SVO_OK;
}

int svo_set_rows(svo_ctx *c, int y0, int y1) {
  if (!c) return SVO_E_INVALID;
  if (y0 < 0 || y1 < y0 || (y0 & 7)) return fail(c, SVO_E_INVALID, "svo_set_rows: need 0 <= y0 <= y1, y0 % 8 == 0");
  c->y0 = y0; c->y1 = y1; c->rows_set = true;
  c->row_step = 1; c->out_y0 = y0; c->n_tile_rows = -1;
  return SVO_OK;
}

int svo_set_stripes(svo_ctx *c, int first_tile_row, int tile_row_step, int n_tile_rows, int out_row0) {
  if (!c) return SVO_E_INVALID;
  if (first_tile_row < 0 || tile_row_step < 1 || n_tile_rows < 0 || out_row0 < 0)
    return fail(c, SVO_E_INVALID, "svo_set_stripes: bad values");
  c->y0 = first_tile_row * 8; c->y1 = 0x7fffffff; c->rows_set = true;
  c->row_step = tile_row_step; c->out_y0 = out_row0; c->n_tile_rows = n_tile_rows;
  return SVO_OK;
}

int svo_set_pipeline(svo_ctx *c, int pipeline) {
  if (!c || pipeline < 0 || pipeline > 2) return fail(c, SVO_E_INVALID, "pipeline must be 0, 1 or 2");
#if !SVO_VARIANTS
  if (pipeline == 2)
    return fail(c, SVO_E_INVALID, "pipeline 2 (staged wavefront tracing, a comparator) is built into libsvohip_variants.so, not into this library");
#endif
  c->pipeline = pipeline;
  return SVO_OK;
}

int svo_set_tuning(svo_ctx *c, int waves_per_cu, int round_threshold_sixteenths) {
  // (16: every burst is one trip -- a round behind every stop, and behind every trip without one: the most rounds there can be)
  if (!c || waves_per_cu < 0 || round_threshold_sixteenths < 0 || round_threshold_sixteenths > 16)
    return fail(c, SVO_E_INVALID, "svo_set_tuning: bad values");
  c->pb.set.waves_per_cu = waves_per_cu;
  c->pb.set.thresh_num = round_threshold_sixteenths;   // 0 = the running kernel's own default
#if SVO_VARIANTS
  c->wf.waves_per_cu = waves_per_cu;
  c->wf.thresh_num = round_threshold_sixteenths ? round_threshold_sixteenths : 12;
#endif
  return SVO_OK;
}

int svo_launch_info(svo_ctx *c, int *waves, int *waves_per_cu, int *round_threshold_sixteenths) {
  if (!c) return SVO_E_INVALID;
  if (waves) *waves = c->pb.buf.last_blocks;
  if (waves_per_cu) *waves_per_cu = c->pb.buf.last_per_cu;
  if (round_threshold_sixteenths) *round_threshold_sixteenths = c->pb.buf.last_thresh;
  return SVO_OK;
}

int svo_set_primary_cache(svo_ctx *c, int enabled) {
  if (!c) return SVO_E_INVALID;
  c->pb.set.kept_mode = enabled != 0 ? 1 : 0;
  if (!enabled) persist_kept_drop(c->pb.buf);
  return SVO_OK;
}

int svo_primary_cache_info(svo_ctx *c, uint64_t *fills, uint64_t *reuses, uint64_t *bytes, int *state) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (fills) *fills = c->pb.set.kept_fills;
  if (reuses) *reuses = c->pb.set.kept_reuses;
  if (bytes) *bytes = (uint64_t)c->pb.buf.kept_cap * 3 * sizeof(uint4);
  if (state) *state = !c->pb.buf.kept_valid ? 0 : (persist_kept_filled(c->pb.buf) ? 2 : 1);
  return SVO_OK;
}

int svo_dense_shade_info(svo_ctx *c, uint64_t *launches, uint64_t *bytes) {
  if (!c) return SVO_E_INVALID;
  if (launches) *launches = c->pb.set.dense_launches;
  if (bytes) *bytes = (uint64_t)c->pb.buf.ray_records * ray_record_bytes(c->pb.set.list_mode != 0) * kHeadSets;
  return SVO_OK;
}

static int ensure_derived(svo_ctx *c);

int svo_set_derived(svo_ctx *c, int mode) {
  if (!c || mode < 0 || mode > 1) return fail(c, SVO_E_INVALID, "svo_set_derived: 0 (records) or 1 (descriptor table)");
  c->derived_mode = mode;
  return SVO_OK;
}

int svo_derived_info(svo_ctx *c, uint64_t *descriptors, uint64_t *bytes, int *walkable, float *build_ms) {
  if (!c) return SVO_E_INVALID;
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, "svo_derived_info: no pool uploaded");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_derived(c);
  if (rc) return rc;
  if (descriptors) *descriptors = c->dt.count;
  if (bytes) *bytes = (uint64_t)c->dt.cap * 2 * sizeof(uint2);
  if (walkable) *walkable = c->dt.ok ? 1 : 0;
  if (build_ms) *build_ms = c->dt.build_ms;
  return SVO_OK;
}

int svo_derived_read(svo_ctx *c, uint64_t first, uint64_t count, void *desc, void *aux) {
  if (!c) return SVO_E_INVALID;
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, "svo_derived_read: no pool uploaded");
  if (count && (!desc || !aux)) return fail(c, SVO_E_INVALID, "svo_derived_read: null buffer");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_derived(c);
  if (rc) return rc;
  if (first > c->dt.count || count > c->dt.count - first) return fail(c, SVO_E_INVALID, "svo_derived_read: range past the table's end");
  if (!count) return SVO_OK;
  HIPCHK(c, hipDeviceSynchronize());   // (a refresh or a build has synchronised its stream; frames only read the table)
  HIPCHK(c, hipMemcpy(desc, c->dt.desc + first, count * sizeof(uint2), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(aux, c->dt.aux + first, count * sizeof(uint2), hipMemcpyDeviceToHost));
  return SVO_OK;
}

int svo_derived_refresh_info(svo_ctx *c, uint64_t *refreshes, uint64_t *states, uint64_t *added, float *gpu_ms) {
  if (!c) return SVO_E_INVALID;
  if (refreshes) *refreshes = c->dt.refreshes;
  if (states) *states = c->dt.refresh_states;
  if (added) *added = c->dt.refresh_added;
  if (gpu_ms) *gpu_ms = c->dt.refresh_ms;
  return SVO_OK;
}

int svo_set_batch(svo_ctx *c, int nframes, uint64_t frame_stride) {
  if (!c || nframes < 1 || nframes > 64) return fail(c, SVO_E_INVALID, "svo_set_batch: 1..64 frames");
  if (nframes > 1 && frame_stride == 0) return fail(c, SVO_E_INVALID, "svo_set_batch: frame_stride must cover one frame's outputs");
  if (frame_stride * (uint64_t)nframes >= (1ull << 32)) return fail(c, SVO_E_INVALID, "svo_set_batch: batch too large for 32-bit output indices");
  c->batch = nframes;
  c->frame_stride = frame_stride;
  return SVO_OK;
}

int svo_set_progressive(svo_ctx *c, int enabled) {
  if (!c) return SVO_E_INVALID;
  c->progressive = enabled ? 1 : 0;
  return SVO_OK;
}

int svo_set_sequence(svo_ctx *c, int nframes, int fresh) {
  if (!c || nframes < 1 || nframes > 4096) return fail(c, SVO_E_INVALID, "svo_set_sequence: 1..4096 frames");
  c->seq = nframes;
  c->seq_fresh = fresh ? 1 : 0;
  return SVO_OK;
}

int svo_set_hit_records(svo_ctx *c, int enabled) {
  if (!c) return SVO_E_INVALID;
  c->write_hits = enabled ? 1 : 0;
  return SVO_OK;
}

int svo_set_stream(svo_ctx *c, void *hip_stream) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  // Between two streams of the caller's there is no synchronisation here: a caller may alternate streams to keep two frames in
  // flight (different output buffers); ordering between them is the caller's business.  Leaving the library's own streams waits for
  // them (below).  They live as long as the context: NULL returns to the current set's.
  if (hip_stream) {
    // leaving the library's own streams: what they still have in flight writes the library's images, which dispatches on the
    // caller's stream may render into next
    if (c->sets.others_inflight || c->sets.is_own_stream(c->stream)) HIPCHK(c, c->sets.sync_own_streams());
    c->stream = (hipStream_t)hip_stream;
  } else {
    c->stream = c->sets.current().stream;
  }
  c->pick.invalidate();
  return SVO_OK;
}

int svo_set_overlap(svo_ctx *c, int sets) {
  if (!c) return SVO_E_INVALID;
  // 0: one set (no alternation); 1: the default number of sets; 2 .. ImageSets::kMax (8): that many
  if (sets < 0 || sets > ImageSets::kMax) return fail(c, SVO_E_INVALID, "svo_set_overlap: 0 (off), 1 (the default number of sets) or 2 .. 8 sets");
  c->sets.overlap = sets == 0 ? 1 : (sets == 1 ? 4 : sets);
  return SVO_OK;
}

int svo_pick_info(svo_ctx *c, int *x, int *y, uint64_t *from_mail, uint64_t *waited) {
  if (!c) return SVO_E_INVALID;
  if (x) *x = c->pick.x;
  if (y) *y = c->pick.y;
  if (from_mail) *from_mail = c->pick.from_mail;
  if (waited) *waited = c->pick.waited;
  return SVO_OK;
}

int svo_set_pick(svo_ctx *c, int x, int y) {
  if (!c) return SVO_E_INVALID;
  if (x < 0 || y < 0) { c->pick.x = -1; c->pick.y = -1; c->pick.follow_centre = false; return SVO_OK; }   // no pick: read-backs wait
  if (c->width > 0 && (x >= c->width || y >= c->height)) return fail(c, SVO_E_INVALID, "svo_set_pick: outside the image");
  c->pick.x = x; c->pick.y = y; c->pick.follow_centre = false;
  return SVO_OK;
}

// ---------------------------------------------------------------- dispatch
// The output row just past the last one a frame writes; f.out_y0 when it writes none (its stripes all start below the image).
// Tile row j covers image rows y0 + 8 j row_step ..., clipped to min(height, y1), and lands at output rows out_y0 + 8 j ...
static int last_written_row(const Frame &f) {
  const long long yend = std::min(f.height, f.y1);
  for (int j = f.tiles_y - 1; j >= 0; j--) {
    const long long gy = (long long)f.y0 + (long long)j * 8 * f.row_step;
    if (gy < yend) return f.out_y0 + j * 8 + (int)std::min<long long>(8, yend - gy);
  }
  return f.out_y0;
}

static int make_frame(svo_ctx *c, const Target &t, Frame &f) {
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, "svo_dispatch: no pool uploaded");
  if (!t.out.color) return fail(c, SVO_E_INVALID, "svo_dispatch: svo_resize not called");
  memcpy(f.cam, t.cam, sizeof f.cam);
  f.width = c->width; f.height = c->height;
  f.y0 = std::min(c->y0, c->height);
  f.y1 = std::min(c->y1, c->height);
  f.row_step = c->row_step;
  f.out_y0 = c->n_tile_rows < 0 ? f.y0 : c->out_y0;
  f.frame_number = t.frame_number; f.render_mode = c->render_mode;
  f.bounces = c->bounces; f.spp = c->spp; f.mirror_mask = c->mirror_mask;
  f.pool_len = (uint32_t)c->pool_len;
  f.dword0 = c->dword0;
  f.tiles_x = (c->width + 7) / 8;
  f.tiles_y = c->n_tile_rows < 0 ? (f.y1 - f.y0 + 7) / 8 : c->n_tile_rows;
  f.ntiles = f.tiles_x * f.tiles_y;
  f.write_hits = (c->write_hits && t.out.hits) ? 1 : 0;
  f.use_beam = 0; f.beam_w = 0; f.beam = nullptr;
  f.progressive = c->progressive;
  f.batch = 1; f.frame_stride = 0; f.seq = 1;
  if (!t.external && c->n_tile_rows > 0) {
    // packed stripes land at output rows out_y0 + 8 j + ly: they must stay inside the library's W x H images
    // (caller-owned gather buffers are the caller's to size, see svo_bind_outputs).  Stripes that write no row fit anywhere.
    // (stripe mode: y1 is the image's height, tiles_y is n_tile_rows)
    const int end = last_written_row(f);
    if (end > f.out_y0 && end > f.height)
      return fail(c, SVO_E_INVALID, "svo_set_stripes: packed stripes do not fit the library-owned images; bind "
                                    "caller-owned outputs that cover out_row0 + 8 * n_tile_rows rows");
  }
  return SVO_OK;
}

// elements per output plane that a launch of `f` may index
static size_t out_elems(const svo_ctx *c, const Frame &f) {
  return std::max((size_t)c->width * (size_t)c->height, (size_t)(f.out_y0 + f.tiles_y * 8) * (size_t)c->width);
}

static int launch_frame_kernels(svo_ctx *c, const Target &t, Frame &f, bool count, uint32_t *color, float *depth, uint4 *hits);

// The descriptor table follows the pool: (re)built at the first dispatch after a pool change.  Every pool mutator has
// synchronised the device, except a caller writing through svo_pool_device_ptr -- so wait for the device here too: no
// frame in flight may still read the table that is replaced.
static int ensure_derived(svo_ctx *c) {
  if (c->derived_valid) return SVO_OK;
  HIPCHK(c, hipDeviceSynchronize());
  hipError_t e = derive::build_table(c->dt, c->d_pool, c->pool_len, c->sets[0].stream);
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string("descriptor table: ") + hipGetErrorString(e));
  c->derived_valid = true;
  return SVO_OK;
}

// Which octree a cast reads: the descriptor table when the context asks for it (derived_mode; a variants build's SVO_DERIVED
// overrides, for A/B runs) and the pool is derivable -- not deeper than 13 levels, not cyclic -- else the records.  The table is
// brought up to date here.
static int pick_walk(svo_ctx *c, bool &walk_table) {
#if SVO_VARIANTS
  static const int env_mode = getenv("SVO_DERIVED") ? atoi(getenv("SVO_DERIVED")) : -1;
#else
  const int env_mode = -1;
#endif
  const int mode = env_mode >= 0 ? env_mode : c->derived_mode;
  walk_table = false;
  if (mode == 0) return SVO_OK;
  const int rc = ensure_derived(c);
  walk_table = rc == SVO_OK && c->dt.ok;
  return rc;
}

static int launch_frame(svo_ctx *c, const Target &t, bool count) {
  Frame f;
  int rc = make_frame(c, t, f);
  if (rc) return rc;
  if (f.ntiles <= 0) return SVO_OK;
  int beam_set = -1;
  if (c->use_beam) HIPCHK(c, beam::enqueue(c->beam, c->d_pool, c->pool_len, f, t.stream, beam_set));
  const int nb = count ? 1 : t.batch;
  if (nb > 1 && !t.external)
    return fail(c, SVO_E_INVALID, "svo_set_batch: a batch renders into caller-owned outputs (svo_bind_outputs)");
  const int last_row = last_written_row(f);
  const bool writes_rows = last_row > f.out_y0;
  // frame k lands frame_stride elements behind frame k - 1: the stride must cover the rows one frame writes, or the
  // frames of the batch overwrite one another
  if (nb > 1 && writes_rows && t.frame_stride < (uint64_t)last_row * (uint64_t)f.width)
    return fail(c, SVO_E_INVALID, "svo_set_batch: frame_stride is smaller than the rows one frame writes");
  if (nb > 1 && f.progressive)
    return fail(c, SVO_E_INVALID, "svo_set_batch: cross-frame accumulation blends into ONE image frame after frame; "
                                  "a batch writes every frame to its own");
  if (nb > 1 && t.cams && c->use_beam)
    return fail(c, SVO_E_INVALID, "svo_ring_submit_cams: the beam pre-pass belongs to one camera; submit such frames one by one");
  const Planes &o = t.out;
  if (f.progressive && (c->seq > 1 || c->seq_fresh) && !count) {
    // a progressive sequence: c->seq frames of the accumulation, frameNumber, frameNumber + 1, ..., into the one image
    // ... starting on a zeroed image when asked (the application's first frames; the image after glTexStorage2D)
    if (c->seq_fresh && writes_rows)
      HIPCHK(c, hipMemsetAsync(o.color + (size_t)f.out_y0 * (size_t)f.width, 0, (size_t)(last_row - f.out_y0) * (size_t)f.width * 4, t.stream));
    Frame probe = f;
    if (c->pipeline == 1 && f.spp <= 1 && persist_can_fold(probe, c->seq, persist_fold_budget())) {
      // the persistent pipeline carries the whole sequence in one launch and blends it in frame order afterwards
      f.seq = c->seq;
      rc = launch_frame_kernels(c, t, f, count, o.color, o.depth, o.hits);
    } else {
      for (int k = 0; k < c->seq && rc == SVO_OK; k++) {
        Frame g = f;
        g.frame_number = f.frame_number + k;
        rc = launch_frame_kernels(c, t, g, count, o.color, o.depth, o.hits);
      }
    }
  } else if (nb > 1 && c->pipeline == 1) {
    // the persistent pipeline takes the whole batch as one launch: its waves go from frame to frame without a tail
    f.batch = nb;
    f.frame_stride = (uint32_t)t.frame_stride;
    rc = launch_frame_kernels(c, t, f, count, o.color, o.depth, o.hits);
  } else {
    for (int k = 0; k < nb && rc == SVO_OK; k++) {
      Frame g = f;
      g.frame_number = f.frame_number + k;
      if (t.cams) { memcpy(g.cam, t.cams[k].cam, sizeof g.cam); g.frame_number = t.cams[k].frame_number; }
      const size_t at = (size_t)k * (size_t)t.frame_stride;
      rc = launch_frame_kernels(c, t, g, count, o.color + at, o.depth + at, o.hits ? o.hits + at : nullptr);
    }
  }
  if (rc == SVO_OK && beam_set >= 0) HIPCHK(c, beam::record(c->beam, beam_set, t.stream));
  return rc;
}

static int ring_copy_cams(void *target);

static int launch_frame_kernels(svo_ctx *c, const Target &t, Frame &f, bool count, uint32_t *color, float *depth, uint4 *hits) {
  int rc = SVO_OK;
  if (count) HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(DeviceCounters), t.stream));
  if (c->pipeline == 1 && !count) {
    bool walk_table;
    if ((rc = pick_walk(c, walk_table)) != SVO_OK) return rc;
    PersistLaunch in;
    in.pool = c->d_pool; in.color = color; in.depth = depth; in.hits = hits; in.out_npix = out_elems(c, f); in.stream = t.stream;
    in.shape = t.shape; in.overlap_sets = t.overlap_sets;
    if (walk_table) { in.desc = c->dt.desc; in.aux = c->dt.aux; in.desc_count = c->dt.count; }
    in.ntab = c->d_ntab;
    if (t.cams) in.fvar = t.cams_slot->d_fvar;
    in.fvar_host = t.cams; in.copy_cams = ring_copy_cams; in.copy_arg = (void *)&t;
    rc = persist_launch(c->pb, f, in);
    if (rc) return fail(c, SVO_E_HIP, std::string("persistent pipeline: ") + hipGetErrorString((hipError_t)rc));
    return SVO_OK;
  }
#if SVO_VARIANTS
  if (c->pipeline == 2 && !count) {
    rc = wavefront_launch(c->wf, c->d_pool, f, color, depth, hits, out_elems(c, f), t.stream);
    if (rc) return fail(c, SVO_E_HIP, std::string("wavefront pipeline: ") + hipGetErrorString((hipError_t)rc));
    return SVO_OK;
  }
#endif
  const int per = (f.ntiles + 7) / 8;
  dim3 grid((unsigned)(per * 8)), block(64);
  if (count)
    hipLaunchKernelGGL(trace_fused_kernel<true>, grid, block, 0, t.stream, c->d_pool, f, color, depth, hits, c->d_counters);
  else
    hipLaunchKernelGGL(trace_fused_kernel<false>, grid, block, 0, t.stream, c->d_pool, f, color, depth, hits, c->d_counters);
  HIPCHK(c, hipGetLastError());
  return SVO_OK;
}

// The frame's pick: a launch of ONE wave on a high-priority stream of its own (pick::launch, svo_fused.hip.h), in front of the
// frame's kernels.  Which frames get one is decided here: those the live shader's store applies to: one sample per pixel, no cross-frame accumulation, no batch, no beam pre-pass (its start distances change the
// iteration count of the hit record), the whole frame (a rank's stripes / a row band may not even contain the pixel).
static int launch_pick(svo_ctx *c, const Target &t) {
  c->pick.invalidate();
  if (c->pick.x < 0 || t.batch != 1 || c->progressive || c->spp != 1 || c->use_beam || c->rows_set || c->n_tile_rows >= 0) return SVO_OK;
  Frame f;
  int rc = make_frame(c, t, f);
  if (rc) return rc;
  if (f.ntiles <= 0 || c->pick.x >= f.width || c->pick.y >= f.height) return SVO_OK;
  HIPCHK(c, pick::launch(c->pick, c->d_pool, f));
  return SVO_OK;
}

int svo_dispatch_async(svo_ctx *c) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  // Up to ImageSets::kMax (8) sets {stream, images} in turn while the library owns them and nothing ties a frame to the image before it: the
  // next frame's persistent waves take the CUs this frame's tail frees (glDispatchCompute only enqueues as well: Renderer.java:118-121).
  ImageSets &sets = c->sets;
  const bool own = !c->external_outputs && sets[0].color && sets.is_own_stream(c->stream);
  const bool overlapped = sets.overlap > 1 && own && c->pipeline == 1 && !c->progressive && c->batch == 1;
  if (overlapped) {
    // nothing of the context names the next set before it is whole: a failed step leaves the current set, c->stream and c->d_* as
    // they were
    HIPCHK(c, sets.take_next((size_t)c->width * (size_t)c->height));
    const ImageSet &s = sets.current();
    c->stream = s.stream;
    c->d_color = s.color; c->d_depth = s.depth; c->d_hits = s.hits;
  }
  Target t = current_target(c);
  if (overlapped) { t.shape = kOverlap; t.overlap_sets = sets.overlap; }   // the launch shape of overlapping one-frame launches
  int rc = launch_pick(c, t);
  if (rc == SVO_OK) {
    rc = launch_frame(c, t, false);
    if (rc) c->pick.invalidate();
  }
  if (overlapped && rc == SVO_OK) {
    ImageSet &s = sets.current();
    HIPCHK(c, hipEventRecord(s.done, s.stream));
    s.used = true;
  }
  return rc;
}

int svo_sync(svo_ctx *c) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->sets.others_inflight) HIPCHK(c, c->sets.sync_own_streams());   // the other sets' frames too
  return SVO_OK;
}

int svo_dispatch(svo_ctx *c) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  const Target t = current_target(c);
  int rc = launch_pick(c, t);
  if (rc) return rc;
  rc = launch_frame(c, t, false);
  if (rc) { c->pick.invalidate(); return rc; }
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->stats.last_dispatch_ms = ms;
  return SVO_OK;
}

int svo_count_frame(svo_ctx *c, svo_stats *out) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  c->pick.invalidate();   // (the counting pass renders into the current images)
  int rc = launch_frame(c, current_target(c), true);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  DeviceCounters h;
  HIPCHK(c, hipMemcpy(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
  c->stats.pixels = h.pixels; c->stats.rays = h.rays; c->stats.nan_rays = h.nan_rays;
  c->stats.iterations = h.iterations; c->stats.alg_bytes = h.alg_bytes; c->stats.max_iter = h.max_iter;
  if (out) *out = c->stats;
  return SVO_OK;
}

int svo_get_stats(svo_ctx *c, svo_stats *out) {
  if (!c || !out) return SVO_E_INVALID;
  *out = c->stats;
  return SVO_OK;
}

int svo_time_frames(svo_ctx *c, int warmup, int iters, float *ms) {
  if (!c || iters <= 0 || !ms) return fail(c, SVO_E_INVALID, "svo_time_frames: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  c->pick.invalidate();
  std::vector<hipEvent_t> ev((size_t)iters + 1, nullptr);
  const Target t = current_target(c);
  int rc = SVO_OK;
  hipError_t e = hipSuccess;
  const char *what = "";
  auto ok = [&](hipError_t r, const char *w) { if (r != hipSuccess && e == hipSuccess) { e = r; what = w; } return r == hipSuccess; };
  for (int i = 0; i < warmup && rc == SVO_OK; i++) rc = launch_frame(c, t, false);
  for (size_t i = 0; i < ev.size() && rc == SVO_OK && e == hipSuccess; i++) ok(hipEventCreate(&ev[i]), "hipEventCreate");
  if (rc == SVO_OK && e == hipSuccess) ok(hipEventRecord(ev[0], c->stream), "hipEventRecord");
  for (int i = 0; i < iters && rc == SVO_OK && e == hipSuccess; i++) {
    rc = launch_frame(c, t, false);
    if (rc == SVO_OK) ok(hipEventRecord(ev[(size_t)i + 1], c->stream), "hipEventRecord");
  }
  (void)hipStreamSynchronize(c->stream);   // also on the error paths: the events must be idle before they go
  for (int i = 0; i < iters && rc == SVO_OK && e == hipSuccess; i++)
    ok(hipEventElapsedTime(&ms[i], ev[(size_t)i], ev[(size_t)i + 1]), "hipEventElapsedTime");
  for (auto &x : ev) if (x) (void)hipEventDestroy(x);
  if (rc != SVO_OK) return rc;
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  c->stats.last_dispatch_ms = ms[iters - 1];
  return SVO_OK;
}


// ---------------------------------------------------------------- ray queries (svo_rays.hip.h)
// the checks both variants share; n > 0 behind it
static int cast_check(svo_ctx *c, const void *rays_, uint32_t n, const void *hits, const char *who) {
  if (n > rays::kMaxRays) return fail(c, SVO_E_TOOLARGE, std::string(who) + ": at most 2^26 rays per call");
  if (!rays_ || !hits) return fail(c, SVO_E_INVALID, std::string(who) + ": null buffer");
  if (!c->d_pool || c->pool_len < 7) return fail(c, SVO_E_NOPOOL, std::string(who) + ": no pool uploaded");
  return SVO_OK;
}

// enqueues the cast of n > 0 rays in device memory on the context's current stream
static int cast_enqueue(svo_ctx *c, const void *d_rays, uint32_t n, void *d_hits, const char *who) {
  bool walk_table;
  const int rc = pick_walk(c, walk_table);
  if (rc) return rc;
  hipError_t e = rays::prepare(c->rs);
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  rays::Args a{};
  a.pool = c->d_pool; a.pool_len = (uint32_t)c->pool_len;
  a.desc = walk_table ? c->dt.desc : nullptr; a.aux = walk_table ? c->dt.aux : nullptr; a.desc_count = walk_table ? c->dt.count : 0u;
  a.ntab = c->d_ntab;
  a.rays = (const float *)d_rays; a.hits = (uint4 *)d_hits; a.n = n;
  a.thresh_num = persist_thresh(c->pb.set);
  e = rays::launch(c->rs, a, walk_table, c->pb.set, c->stream);
  if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return SVO_OK;
}

int svo_cast_rays_device(svo_ctx *c, const void *d_rays, uint32_t n, void *d_hits) {
  if (!c) return SVO_E_INVALID;
  if (n == 0) return SVO_OK;
  int rc = cast_check(c, d_rays, n, d_hits, "svo_cast_rays_device");
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return cast_enqueue(c, d_rays, n, d_hits, "svo_cast_rays_device");
}

int svo_cast_rays(svo_ctx *c, const float *rays_, uint32_t n, svo_hit *hits) {
  if (!c) return SVO_E_INVALID;
  if (n == 0) return SVO_OK;
  int rc = cast_check(c, rays_, n, hits, "svo_cast_rays");
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rays::State &s = c->rs;
  if (s.cap < n) {
    // (the staging buffers are idle between calls: every call that used them has waited for its cast before it returned)
    float *nr = nullptr; uint4 *nh = nullptr;
    hipError_t e = hipMalloc((void **)&nr, (size_t)n * 6 * sizeof(float));
    if (e == hipSuccess && (e = hipMalloc((void **)&nh, (size_t)n * sizeof(uint4))) != hipSuccess) (void)hipFree(nr);
    if (e != hipSuccess) return fail(c, SVO_E_HIP, std::string("svo_cast_rays: staging buffers: ") + hipGetErrorString(e));
    if (s.d_rays) (void)hipFree(s.d_rays);
    if (s.d_hits) (void)hipFree(s.d_hits);
    s.d_rays = nr; s.d_hits = nh; s.cap = n;
  }
  HIPCHK(c, hipMemcpyAsync(s.d_rays, rays_, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  rc = cast_enqueue(c, s.d_rays, n, s.d_hits, "svo_cast_rays");
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }   // (the copy in may still read the caller's rays)
  HIPCHK(c, hipMemcpyAsync(hits, s.d_hits, (size_t)n * sizeof(uint4), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SVO_OK;
}

int svo_cast_info(svo_ctx *c, uint64_t *calls, uint64_t *rays_, int *waves, int *walk, float *gpu_ms) {
  if (!c) return SVO_E_INVALID;
  if (calls) *calls = c->rs.calls;
  if (rays_) *rays_ = c->rs.rays;
  if (waves) *waves = c->rs.waves;
  if (walk) *walk = c->rs.walk;
  if (gpu_ms) { HIPCHK(c, hipSetDevice(c->device)); *gpu_ms = rays::last_ms(c->rs); }
  return SVO_OK;
}

}  // extern "C"
// ---------------------------------------------------------------- frames in flight behind the boundary: the ring's functions
#define SVO_RING_FUNCTIONS 1
#include "svo_ring.hip.h"
extern "C" {

// ---------------------------------------------------------------- device memory shared between the ranks of one node
int svo_dev_alloc(svo_ctx *c, uint64_t nbytes, void **dptr) {
  if (!c || !dptr || nbytes == 0) return fail(c, SVO_E_INVALID, "svo_dev_alloc: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(dptr, nbytes));
  c->dev_allocs.push_back(*dptr);
  HIPCHK(c, hipMemset(*dptr, 0, nbytes));
  HIPCHK(c, hipDeviceSynchronize());
  return SVO_OK;
}
int svo_dev_free(svo_ctx *c, void *dptr) {
  if (!c) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  for (auto &p : c->dev_allocs)
    if (p && p == dptr) { p = nullptr; HIPCHK(c, hipFree(dptr)); return SVO_OK; }
  return dptr ? fail(c, SVO_E_INVALID, "svo_dev_free: not allocated by this context") : SVO_OK;
}
int svo_dev_read(svo_ctx *c, const void *dptr, void *host, uint64_t nbytes) {
  if (!c || !dptr || !host) return fail(c, SVO_E_INVALID, "svo_dev_read: null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(host, dptr, nbytes, hipMemcpyDeviceToHost));
  return SVO_OK;
}
int svo_ipc_export(svo_ctx *c, void *dptr, void *handle64) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  if (!c || !dptr || !handle64) return fail(c, SVO_E_INVALID, "svo_ipc_export: null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  HIPCHK(c, hipIpcGetMemHandle(&h, dptr));
  memcpy(handle64, &h, sizeof h);
  return SVO_OK;
}
int svo_ipc_open(svo_ctx *c, const void *handle64, void **dptr) {
  if (!c || !dptr || !handle64) return fail(c, SVO_E_INVALID, "svo_ipc_open: null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, sizeof h);
  HIPCHK(c, hipIpcOpenMemHandle(dptr, h, hipIpcMemLazyEnablePeerAccess));
  c->ipc_opened.push_back(*dptr);
  return SVO_OK;
}
int svo_ipc_close(svo_ctx *c, void *dptr) {
  if (!c || !dptr) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  for (auto &p : c->ipc_opened)
    if (p == dptr) { p = nullptr; HIPCHK(c, hipIpcCloseMemHandle(dptr)); return SVO_OK; }
  return fail(c, SVO_E_INVALID, "svo_ipc_close: not opened by this context");
}

// ---------------------------------------------------------------- readback
static int read_rows(svo_ctx *c, void *dst, const void *src, size_t elem) {
  if (!dst) return fail(c, SVO_E_INVALID, "readback: null buffer");
  if (!src) return fail(c, SVO_E_INVALID, "readback before svo_resize");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, src, (size_t)c->width * (size_t)c->height * elem, hipMemcpyDeviceToHost));
  return SVO_OK;
}
int svo_read_color(svo_ctx *c, void *rgba8) { return c ? read_rows(c, rgba8, c->d_color, 4) : SVO_E_INVALID; }
int svo_read_depth(svo_ctx *c, float *depth) { return c ? read_rows(c, depth, c->d_depth, 4) : SVO_E_INVALID; }
int svo_read_hits(svo_ctx *c, svo_hit *hits) { return c ? read_rows(c, hits, c->d_hits, 16) : SVO_E_INVALID; }

int svo_read_beam(svo_ctx *c, float *beam) {
  if (!c || !beam) return fail(c, SVO_E_INVALID, "svo_read_beam: null buffer");
  const beam::State &b = c->beam;
  if (!b.frames || !b.cap) return fail(c, SVO_E_INVALID, "svo_read_beam: no frame was dispatched with use_beam");
  HIPCHK(c, hipSetDevice(c->device));
  const int set = (int)((b.frames - 1) % beam::kSets);
  // the frame that made this image may have run on another stream than the current one (frames in flight)
  if (b.used[set]) HIPCHK(c, hipEventSynchronize(b.done[set]));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)((c->width + kBeamBlock - 1) / kBeamBlock) * (size_t)((c->height + kBeamBlock - 1) / kBeamBlock);
  HIPCHK(c, hipMemcpy(beam, b.img[set], std::min(n, b.cap) * sizeof(float), hipMemcpyDeviceToHost));
  return SVO_OK;
}

int svo_read_pixel(svo_ctx *c, int x, int y, void *rgba8, float *depth, svo_hit *hit) {
  if (!c) return SVO_E_INVALID;
  if (x < 0 || y < 0 || x >= c->width || y >= c->height) return fail(c, SVO_E_INVALID, "svo_read_pixel: outside the image");
  if (!c->d_color) return fail(c, SVO_E_INVALID, "readback before svo_resize");
  HIPCHK(c, hipSetDevice(c->device));
  pick::State &p = c->pick;
  if (p.live && x == p.live_x && y == p.live_y && p.mail && (!hit || (c->write_hits && c->d_hits))) {
    // the pick pixel of the last dispatch: answered from its mail slot.  Should the pick stream run dry without the word, the
    // waiting path answers.
    bool got = false;
    const hipError_t q = pick::poll(p, got, rgba8, depth, hit);
    if (q != hipSuccess) return fail(c, SVO_E_HIP, std::string("svo_read_pixel: ") + hipGetErrorString(q));
    if (got) return SVO_OK;
  }
  p.waited++;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t o = (size_t)y * (size_t)c->width + (size_t)x;
  if (rgba8) HIPCHK(c, hipMemcpy(rgba8, c->d_color + o, 4, hipMemcpyDeviceToHost));
  if (depth) HIPCHK(c, hipMemcpy(depth, c->d_depth + o, 4, hipMemcpyDeviceToHost));
  if (hit) {
    if (!c->d_hits) return fail(c, SVO_E_INVALID, "svo_read_pixel: no hit image bound");
    HIPCHK(c, hipMemcpy(hit, c->d_hits + o, 16, hipMemcpyDeviceToHost));
  }
  return SVO_OK;
}

int svo_output_device_ptrs(svo_ctx *c, void **color, void **depth, void **hits) {
  if (!c) return SVO_E_INVALID;
  if (color) *color = c->d_color;
  if (depth) *depth = c->d_depth;
  if (hits) *hits = c->d_hits;
  return SVO_OK;
}

}  // extern "C"
#include "svo_group.hip.h"
extern "C" {

#ifdef SVO_STAMPS
// diagnostic builds only: the diagnostics words of the persistent pipeline's last counter set (16 x u64, then the
// 64-word histograms of lanes traversing per trip and of lanes in the POP section, 8 x u64 of a round's parts): 704 bytes
int svo_debug_heads(svo_ctx *c, void *out) {
  if (!c || !out || !c->pb.buf.heads) return SVO_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, c->pb.buf.heads + (size_t)((c->pb.buf.frames - 1) % kHeadSets) * kHeadWords + 8 * kHeadStride, 704, hipMemcpyDeviceToHost));
  return SVO_OK;
}
#endif

}  // extern "C"
