// svo_rays.hip.h -- svo_cast_rays: caller-supplied rays through the octree.
//
// The persistent waves of pipeline 1 (svo_persistent.hip.h) without a camera, a pixel or a path: a lane owns one RAY at a
// time -- six floats {origin, direction} in the shader's space, taken by index from the caller's array -- casts it exactly
// as svotrace.comp:main casts a primary ray (normalize3, intersectOctree with coneTrace = false and t_start = 0) and
// stores the svo_hit a frame kernel writes for a pixel's first cast at the ray's index.  Nothing is shaded and no ray
// follows from another, so a round is: stopped lanes store their record, idle lanes draw the next indices from ONE
// counter (one atomic per wave and round: ballot + prefix count, as persist_body refills), the new rays are set up, and
// the wave runs trips (the Walk's own loop: ByteWalk over the pool's records, DescWalk over the descriptor table) until
// enough lanes have stopped.  Once the counter has passed the last ray the drain rule of persist_body applies: a tail does
// not wait for its longest ray.
//
// Not here: cone rays, a per-ray t_max or any-hit early-out (they change `iter`), a hit position or a decoded normal in
// the record (o + t d; raw_normal), the N-GPU group (include/svo_hip.h).
#pragma once
#include "svo_persistent.hip.h"

namespace svo {
namespace rays {

constexpr uint32_t kMaxRays = 1u << 26;   // per call: 1.5 GiB of rays, 1 GiB of records
constexpr int kCounters = 8;              // work counters, one per call in flight, reused round-robin behind an event
constexpr int kCounterStride = 32;        // words: a 128-byte line each (svo_persistent.hip.h::kHeadStride)

struct Args {
  const uint8_t *pool;
  uint32_t pool_len;
  // interior-descriptor table (svo_derive.hip.h); only read by the DescWalk kernel
  const uint2 *desc;
  const uint2 *aux;
  uint32_t desc_count;
  const float4 *ntab;
  const float *rays;    // n x {ox, oy, oz, dx, dy, dz}
  uint4 *hits;          // n records, by ray index
  uint32_t n;
  uint32_t *head;       // ray indices drawn so far (zeroed in front of the launch)
  int thresh_num;       // a round starts once active lanes <= thresh_num/16 of those active at its start
};

// what Walk::setup(const PersistArgs &) reads, from the ray launch's arguments
__device__ __forceinline__ void setup(ByteWalk &w, const Args &a) {
  w.pool = make_bufpool(a.pool, a.pool_len);
  w.root = load_record(w.pool, 0u);
}
__device__ __forceinline__ void setup(DescWalk &w, const Args &a) {
  w.pool = make_bufpool(a.pool, a.pool_len);
  w.tab = make_desctab(a.desc, a.aux, a.desc_count, a.ntab);
  const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(w.tab.rsrc, (int)kDescRoot, 0, 0);
  w.rootd = make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)r.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y));
}

template <class Walk>
__global__ __launch_bounds__(64, WalkWaves<Walk>::value) void rays_kernel(const Args a) {
  __shared__ typename Walk::Stack stk;
  const uint32_t lane = threadIdx.x;
  Walk walk;
  setup(walk, a);

  typename Walk::State t;
  int status = ST_IDLE;
  uint32_t k = 0;      // the lane's ray
  bool more = true;    // wave-uniform: the counter has not passed the last ray yet

  for (;;) {
    // ---------------- stopped lanes: the record, packed as persist_body packs a.hits[pix]
    if (status >= ST_HIT) {
      const Cast c = walk.result(t, status);
      status = ST_IDLE;
      uint4 h;
      h.x = c.hit ? c.pointer : 0u;
      h.y = c.hit ? ((c.raw & 0xffffu) | ((c.value & 0xffu) << 16) | ((c.level & 0xffu) << 24)) : 0u;
      h.z = c.iter;
      h.w = c.hit ? __float_as_uint(c.t) : 0u;
      a.hits[k] = h;
    }
    // ---------------- refill idle lanes: ballot + prefix count, one atomic per wave
    bool ninit = false;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    if (more) {
      const unsigned long long idle = __ballot(status == ST_IDLE);
      if (idle != 0ull) {
        const uint32_t n = (uint32_t)__builtin_popcountll(idle);
        const int leader = __builtin_ctzll(idle);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(a.head, n);
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);   // wave-uniform, and the compiler knows it
        const uint32_t slot =
            base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (status == ST_IDLE && slot < a.n) {
          k = slot;
          const float *r = a.rays + (size_t)k * 6u;   // (4-byte aligned is all the caller owes)
          o = mk(r[0], r[1], r[2]);
          d = normalize3(mk(r[3], r[4], r[5]));
          ninit = true;
          status = ST_ACTIVE;   // taken (the set-up below gives the real status)
        }
        // (n <= 2^26 and every wave overshoots by at most 64 once: the counter cannot wrap)
        if (base + n >= a.n) more = false;
      }
    }
    // ---------------- set up the new rays
    if (ninit) {
      status = walk.init(t, o, d, false, 0.0f);
      walk.fresh_stack(stk, lane);
    }
    if (__ballot(status != ST_IDLE) == 0ull) {
      if (more) continue;
      break;
    }
    // ---------------- traverse until enough lanes have stopped to make a round worthwhile (persist_body's rule and drain)
    const unsigned long long act = __ballot(status == ST_ACTIVE);
    const int active0 = __builtin_popcountll(act);
    if (active0 == 0) continue;   // every new ray ended in its set-up (all-NaN rays): straight to their records
    const int drained = (active0 * SVO_DRAIN_NUM) / 16 < active0 - 1 ? (active0 * SVO_DRAIN_NUM) / 16 : active0 - 1;
    const int threshold = __builtin_amdgcn_readfirstlane(more ? (active0 * a.thresh_num) / 16 : drained);
    walk.run(stk, lane, t, status, act, threshold, 0ull, nullptr);
  }
}

// The host side's scratch: counters and their events, the staging buffers of the host variant, what svo_cast_info reports.
struct State {
  uint32_t *heads = nullptr;            // kCounters counters, kCounterStride words apart
  hipEvent_t e0[kCounters] = {}, e1[kCounters] = {};   // around the call that used the counter last (e1: its re-use waits for it)
  bool used[kCounters] = {};
  unsigned next = 0;
  int last = -1;                        // the counter of the last call, -1 = none yet
  float *d_rays = nullptr;              // staging of svo_cast_rays, grown as needed
  uint4 *d_hits = nullptr;
  uint32_t cap = 0;                     // rays they have room for
  int cus = 0, fit[2] = {0, 0};         // CUs; waves per CU that fit: record walk / descriptor walk
  uint64_t calls = 0, rays = 0;
  int waves = 0, walk = 0;
};

inline void free_state(State &s) {
  if (s.heads) (void)hipFree(s.heads);
  if (s.d_rays) (void)hipFree(s.d_rays);
  if (s.d_hits) (void)hipFree(s.d_hits);
  for (auto &e : s.e0) if (e) (void)hipEventDestroy(e);
  for (auto &e : s.e1) if (e) (void)hipEventDestroy(e);
  s = State();
}

// counters, events and the launch shape's figures, at the first call
inline hipError_t prepare(State &s) {
  hipError_t e;
  if (!s.heads && (e = hipMalloc((void **)&s.heads, kCounters * kCounterStride * sizeof(uint32_t))) != hipSuccess) return e;
  for (int i = 0; i < kCounters; i++) {
    if (!s.e0[i] && (e = hipEventCreate(&s.e0[i])) != hipSuccess) return e;
    if (!s.e1[i] && (e = hipEventCreate(&s.e1[i])) != hipSuccess) return e;
  }
  if (s.cus == 0) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    // what a waiting dispatch fills a CU with (persist_prepare), and no more than fit of this kernel
    int pk = 0, rk = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pk, persist_kernel<0, ByteWalk>, 64, 0) != hipSuccess || pk < 1) pk = 16;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&rk, rays_kernel<ByteWalk>, 64, 0) != hipSuccess || rk < 1) rk = 16;
    s.fit[0] = std::min(pk, rk);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pk, persist_kernel<0, DescWalk>, 64, 0) != hipSuccess || pk < 1) pk = 16;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&rk, rays_kernel<DescWalk>, 64, 0) != hipSuccess || rk < 1) rk = 16;
    s.fit[1] = std::min(pk, rk);
    s.cus = cus > 0 ? cus : 256;
  }
  return hipSuccess;
}

// Enqueues one cast of a.n rays (> 0) on `stream`: the counter's turn, its zeroing, the launch, the events around it.
// Waves per CU: the host's figure (svo_set_tuning), else what a waiting dispatch uses -- persist_plan's rule for a launch
// that has the GPU to itself.  a.head is set here.
inline hipError_t launch(State &s, Args a, bool walk_table, const PersistSettings &set, hipStream_t stream) {
  hipError_t e;
  const int i = (int)(s.next % kCounters);
  if (s.used[i] && (e = hipStreamWaitEvent(stream, s.e1[i], 0)) != hipSuccess) return e;
  a.head = s.heads + i * kCounterStride;
  const int per_cu = persist_waves_per_cu(set, s.fit[walk_table ? 1 : 0]);
  const uint64_t want = ((uint64_t)a.n + 63u) / 64u, room = (uint64_t)per_cu * (uint64_t)s.cus;
  const int waves = (int)std::min(want, room);
  if ((e = hipEventRecord(s.e0[i], stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.head, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (walk_table) hipLaunchKernelGGL(rays_kernel<DescWalk>, dim3((unsigned)waves), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(rays_kernel<ByteWalk>, dim3((unsigned)waves), dim3(64), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipEventRecord(s.e1[i], stream)) != hipSuccess) return e;
  s.used[i] = true; s.next++; s.last = i;
  s.calls++; s.rays += a.n; s.waves = waves; s.walk = walk_table ? 1 : 0;
  return hipSuccess;
}

// GPU time of the last call, 0 until it has completed; never waits
inline float last_ms(const State &s) {
  if (s.last < 0) return 0.0f;
  const hipError_t q = hipEventQuery(s.e1[s.last]);
  if (q != hipSuccess) { (void)hipGetLastError(); return 0.0f; }
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s.e0[s.last], s.e1[s.last]) != hipSuccess) { (void)hipGetLastError(); return 0.0f; }
  return ms;
}

}  // namespace rays
}  // namespace svo
