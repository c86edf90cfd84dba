// svo_brush.hip.h -- an SDF brush stroke on the device pool (svo_brush_sphere / svo_brush_box, include/svo_hip.h):
// Octree.useSDFBrush + subdivideNode + updateExistingNodeBounds (Octree.java:672-885) with sdf/Sphere.java, sdf/Box.java,
// Util.getIntDistance / packNormal (Util.java:140-159).  Included by svo_hip.hip.
//
// The reference's recursion is sequential and appends at memOffset; what it leaves is a function of the tree alone:
//   * what happens to a visited node depends on the SDF, the node's cube, whether it is a leaf, the brush value and the
//     node's own value byte before the stroke.  A node the stroke creates is a leaf with its parent's old value;
//   * the voxel march's three flags are ORs over its (i, j) rows: k restarts in every row, and the early break fires only
//     once volume and air are both seen, where bordersVolume no longer decides anything;
//   * sibling updates touch different 2-bit fields of the parent's mask, start0 is a min, end0 a max under the constant
//     filter end0 < start1; only the allocation order is sequential, and it is the DFS preorder of the subdividing nodes.
// So a stroke is: PLAN (nothing is written to the pool) -- per level a march launch (lanes take rows, several small nodes per
// wave, many waves per large node) and a decide launch that emits the next level's work items, a node's eight children
// contiguous; a bottom-up pass that sums the bytes every subtree appends; a top-down pass that hands out offsets (own block
// at base, child n behind it and behind the subtrees of the children before it) -- then the host grows the pool once, and
// one WRITE launch stores every byte of the new records and patches the old ones, every parent writing its mask once from
// its eight children's decisions.  A plan that fails (a record outside the pool, too many work items, a result of 2^31
// bytes) leaves the pool as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace svo {
namespace brush {

constexpr uint8_t kDeleteValue = 127;          // Constants.java:16
constexpr int kMarchDistanceMinCutoff = 5;     // Constants.java:32
constexpr int kMaxLevels = 20;                 // world_size <= 32768 halves to 0 in 16 steps
constexpr int kMaxWorld = 32768;

struct Sdf {
  int kind;              // 0: sdf/Sphere.java, 1: sdf/Box.java
  int o[3], mn[3], mx[3];
  int r;                 // sphere
  int b[3];              // box: width, height, depth
};

// one visited node
struct Item {
  uint32_t ptr;          // its record (a node the stroke creates: handed out by offsets_kernel)
  uint32_t parent;       // item of its parent (the root: itself)
  int32_t x, y, z;
  uint32_t first_child;  // kRecurse / kSubdivide: the item of child 0, the others follow
  uint32_t sub_bytes;    // bytes the stroke appends for the subtree below (and including) this node's subdivision
  uint32_t base;         // where those bytes start
  uint32_t bits;
  uint32_t pad;          // (40 bytes: 8-byte aligned rows)
};
// Item::bits
constexpr uint32_t kValueMask = 0xffu;                               // the value byte before the stroke
constexpr uint32_t kVolume = 1u << 8, kBorders = 1u << 9, kAir = 1u << 10;   // the march's flags
constexpr uint32_t kLeaf = 1u << 11, kNew = 1u << 12, kShort = 1u << 13;     // kShort: a record of 3 bytes or 1 byte
constexpr uint32_t kDecShift = 14, kDecMask = 7u << kDecShift;
constexpr uint32_t kChildShift = 17;                                 // childNumber, 3 bits
constexpr uint32_t kNormalShift = 20;                                // packed normal of a new surface leaf (<= 999)
enum : uint32_t { kNone = 0, kSetValue = 1, kFill = 2, kRecurse = 3, kSubdivide = 4 };

// device counters
enum : uint32_t { kCtrItems = 0, kCtrFlags = 1, kCtrStart0 = 2, kCtrEnd0 = 3, kCtrLo = 4, kCtrHi = 5, kCtrSubdivided = 6, kCtrWords = 8 };
enum : uint32_t { kFlagBounds = 1u, kFlagItems = 2u, kFlagShortLeaf = 4u };

__host__ __device__ inline long long isqrt_floor(long long n) {
  long long m = (long long)sqrt((double)n);
  while (m * m > n) m--;
  while ((m + 1) * (m + 1) <= n) m++;
  return m;
}

// Sphere.distance: Math.round(sqrt(n)) - radius; the square root of an integer is never k + 1/2, so rounding is the integer
// comparison n - m^2 > m.  Box.distance: (int)sqrt of the clipped extents, the FULL extents subtracted (Box.java:29-43).
__host__ __device__ inline int sdf_distance(const Sdf &s, int x, int y, int z) {
  if (s.kind == 0) {
    const long long dx = (long long)x - s.o[0], dy = (long long)y - s.o[1], dz = (long long)z - s.o[2];
    const long long n = dx * dx + dy * dy + dz * dz;
    const long long m = isqrt_floor(n);
    return (int)(m + (n - m * m > m ? 1 : 0)) - s.r;
  }
  long long q0 = (long long)abs(x - s.o[0]) - s.b[0], q1 = (long long)abs(y - s.o[1]) - s.b[1], q2 = (long long)abs(z - s.o[2]) - s.b[2];
  q0 = q0 < 0 ? 0 : q0; q1 = q1 < 0 ? 0 : q1; q2 = q2 < 0 ? 0 : q2;
  return (int)isqrt_floor(q0 * q0 + q1 * q1 + q2 * q2);
}

// Java's (int) of a double (JLS 5.1.3)
__host__ __device__ inline int java_d2i(double v) {
  if (v != v) return 0;
  if (v >= 2147483647.0) return 2147483647;
  if (v <= -2147483648.0) return -2147483647 - 1;
  return (int)v;
}

// SignedDistanceField.normal: Util.packNormal(Util.normalize(diff)) in IEEE double, the divide before the multiply
__host__ __device__ inline uint32_t sdf_normal(const Sdf &s, int x, int y, int z, bool face_outwards) {
  const int p[3] = {x, y, z};
  int d[3];
  for (int i = 0; i < 3; i++) d[i] = face_outwards ? p[i] - s.o[i] : s.o[i] - p[i];
  const double len = sqrt((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1] + (double)d[2] * (double)d[2]);
  int n[3];
  for (int i = 0; i < 3; i++) {
    const double q = (double)d[i] / len;
    n[i] = java_d2i(q * 9) / 2 + 5;
  }
  return (uint32_t)(uint16_t)(int16_t)(n[0] + n[1] * 10 + n[2] * 100);
}

__device__ __forceinline__ int be32(const uint8_t *p) {
  return (int)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}
__device__ __forceinline__ uint32_t rec_size(uint32_t tag) { return tag == 1u ? 3u : (tag == 3u ? 1u : 7u); }

// ---------------------------------------------------------------------------------------------------------------------
// The march of the items [lo, lo + n), all of edge `size`.  `lanes` (a power of two, 1..64) lanes share an item and take its
// rows in turn; blockIdx.y names a chunk of lanes * iters rows, so that a large node is marched by many waves.  One wave per
// block.
__global__ __launch_bounds__(64) void march_kernel(Item *items, uint32_t lo, uint32_t n, int size, Sdf s, uint32_t lanes, uint32_t iters) {
  const uint32_t lane = threadIdx.x, per_wave = 64u / lanes, sub = lane & (lanes - 1u), grp = lane / lanes;
  const uint32_t k = blockIdx.x * per_wave + grp;
  bool valid = k < n;
  Item it{};
  if (valid) it = items[lo + k];
  // intersectAABB (Util.java:5-9), inclusive on both sides
  if (valid)
    valid = it.x <= s.mx[0] && it.x + size >= s.mn[0] && it.y <= s.mx[1] && it.y + size >= s.mn[1] && it.z <= s.mx[2] && it.z + size >= s.mn[2];
  const int i0 = max(it.x, s.mn[0]), j0 = max(it.y, s.mn[1]), k0 = max(it.z, s.mn[2]);
  const int ni = valid ? it.x + size - i0 : 0, nj = valid ? it.y + size - j0 : 0, kend = it.z + size;
  const uint32_t rows = (uint32_t)ni * (uint32_t)nj;   // <= 2^30
  // another wave of this node may already have seen both
  if (valid && gridDim.y > 1 && (it.bits & (kVolume | kAir)) == (kVolume | kAir)) valid = false;
  const unsigned long long gmask = (lanes == 64u ? ~0ull : ((1ull << lanes) - 1ull)) << (grp * lanes);
  bool v = false, b = false, a = false, done = false;
  const uint64_t first = (uint64_t)blockIdx.y * lanes * iters;
  for (uint32_t t = 0;; t++) {
    const uint64_t r = first + (uint64_t)t * lanes + sub;
    const bool work = valid && !done && t < iters && r < rows;
    if (!__any(work)) break;
    if (work) {
      const int i = i0 + (int)((uint32_t)r / (uint32_t)nj), j = j0 + (int)((uint32_t)r % (uint32_t)nj);
      for (int kk = k0; kk < kend; kk++) {
        const int dist = sdf_distance(s, i, j, kk);
        const int ad = dist < 0 ? -dist : dist;
        if (dist <= 0) v = true;
        if (dist == 1 || dist == 0) b = true;
        if (dist > 0) a = true;
        int march = ad - 2;
        if (march < kMarchDistanceMinCutoff) march = 0;
        kk += march;
        if (v && a) break;
      }
    }
    const unsigned long long bv = __ballot(v), ba = __ballot(a);
    done = (bv & gmask) != 0ull && (ba & gmask) != 0ull;
  }
  const unsigned long long bv = __ballot(v), bb = __ballot(b), ba = __ballot(a);
  if (k < n && sub == 0u) {
    const uint32_t f = ((bv & gmask) ? kVolume : 0u) | ((bb & gmask) ? kBorders : 0u) | ((ba & gmask) ? kAir : 0u);
    if (f) atomicOr(&items[lo + k].bits, f);
  }
}

// The eight children of the record at `ptr` as the leaf mask `mask` lays them out (forEachChild, Octree.java:901-923): false
// when one of them -- its whole record, or (!whole) its value byte -- lies outside the pool
__device__ inline bool children_at(const uint8_t *pool, uint32_t pool_len, uint32_t ptr, uint32_t mask, bool whole, uint32_t cptr[8],
                                   uint32_t ctag[8]) {
  long long cp = (long long)ptr + (long long)be32(pool + ptr + 1);
  for (uint32_t c = 0; c < 8u; c++) {
    const uint32_t tag = (mask >> (2u * c)) & 3u, sz = rec_size(tag);
    if (cp < 0 || cp + (long long)(whole ? sz : 1u) > (long long)pool_len) return false;
    cptr[c] = (uint32_t)cp; ctag[c] = tag;
    cp += sz;
  }
  return true;
}
__device__ inline bool children_of(const uint8_t *pool, uint32_t pool_len, uint32_t ptr, uint32_t cptr[8], uint32_t ctag[8]) {
  return children_at(pool, pool_len, ptr, ((uint32_t)pool[ptr + 5] << 8) | (uint32_t)pool[ptr + 6], true, cptr, ctag);
}

// What happens to each item of [lo, lo + n) (the private useSDFBrush, Octree.java:710-827), and its children's items
__global__ __launch_bounds__(256) void decide_kernel(const uint8_t *pool, uint32_t pool_len, Item *items, uint32_t lo, uint32_t n, int size,
                                                     int level, int value, int max_lod, uint32_t cap, uint32_t *ctr, Sdf s) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t i = lo + t;
  Item it = items[i];
  const bool V = it.bits & kVolume, B = it.bits & kBorders, A = it.bits & kAir, leaf = it.bits & kLeaf;
  const uint32_t vb = it.bits & kValueMask;
  uint32_t dec = kNone;
  if (V && A) dec = leaf ? kSubdivide : kRecurse;
  else if (V) dec = leaf ? ((B && size > 1 && value != 0) ? kSubdivide : kSetValue) : kFill;
  else if (B && size > 1) dec = leaf ? kSubdivide : kRecurse;
  if (dec == kSubdivide && (uint32_t)value == vb) dec = kNone;   // subdivideNode: value == currentValue
  if (dec == kSubdivide && (it.bits & kShort)) {                 // a 3-byte or 1-byte record has no room for a child pointer
    atomicOr(ctr + kCtrFlags, kFlagShortLeaf);
    dec = kNone;
  }
  uint32_t cptr[8], ctag[8];
  if (dec == kFill || dec == kRecurse) {
    if (!children_of(pool, pool_len, it.ptr, cptr, ctag)) { atomicOr(ctr + kCtrFlags, kFlagBounds); dec = kNone; }
  }
  it.first_child = 0;
  if (dec == kRecurse || dec == kSubdivide) {
    const uint32_t first = atomicAdd(ctr + kCtrItems, 8u);
    if ((uint64_t)first + 8u > cap) {
      atomicOr(ctr + kCtrFlags, kFlagItems);
      dec = kNone;
    } else {
      it.first_child = first;
      const int cs = size / 2;
      const bool child_short = level + 1 == max_lod;
      uint32_t normal = 0;
      if (dec == kSubdivide && child_short) normal = sdf_normal(s, it.x, it.y, it.z, value != 0);
      for (uint32_t c = 0; c < 8u; c++) {
        Item ch{};
        ch.parent = i;
        ch.x = it.x + (int)(c & 1u) * cs; ch.y = it.y + (int)((c >> 1) & 1u) * cs; ch.z = it.z + (int)((c >> 2) & 1u) * cs;
        if (dec == kRecurse) {
          ch.ptr = cptr[c];
          ch.bits = (uint32_t)pool[cptr[c]] | (ctag[c] ? kLeaf : 0u) | ((ctag[c] & 1u) ? kShort : 0u) | (c << kChildShift);
        } else {
          ch.bits = vb | kLeaf | kNew | (child_short ? kShort : 0u) | (c << kChildShift) | (normal << kNormalShift);
        }
        items[first + c] = ch;
      }
    }
  }
  it.bits = (it.bits & ~kDecMask) | (dec << kDecShift);
  items[i] = it;
}

__device__ __forceinline__ uint32_t decision(const Item &it) { return (it.bits & kDecMask) >> kDecShift; }

// bottom-up: bytes appended by the subtree of each item of [lo, lo + n)
__global__ __launch_bounds__(256) void sum_kernel(Item *items, uint32_t lo, uint32_t n) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  Item &it = items[lo + t];
  const uint32_t dec = decision(it);
  uint32_t sum = 0;
  if (dec == kRecurse || dec == kSubdivide) {
    if (dec == kSubdivide) sum = 8u * ((items[it.first_child].bits & kShort) ? 3u : 7u);
    for (uint32_t c = 0; c < 8u; c++) sum += items[it.first_child + c].sub_bytes;
  }
  it.sub_bytes = sum;
}

// top-down: the DFS preorder of the subdividing nodes (own block at base, then the children's subtrees in order)
__global__ __launch_bounds__(256) void offsets_kernel(Item *items, uint32_t lo, uint32_t n) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const Item it = items[lo + t];
  const uint32_t dec = decision(it);
  if (dec != kRecurse && dec != kSubdivide) return;
  uint32_t run = it.base;
  if (dec == kSubdivide) {
    const uint32_t sz = (items[it.first_child].bits & kShort) ? 3u : 7u;
    for (uint32_t c = 0; c < 8u; c++) items[it.first_child + c].ptr = it.base + c * sz;
    run += 8u * sz;
  }
  for (uint32_t c = 0; c < 8u; c++) {
    Item &ch = items[it.first_child + c];
    ch.base = run;
    run += ch.sub_bytes;
  }
}

// updateExistingNodeBounds (Octree.java:690-698)
__device__ __forceinline__ void note_bounds(uint32_t *ctr, uint32_t start1, uint32_t s0, uint32_t e0) {
  atomicMin(ctr + kCtrStart0, s0);
  if (e0 < start1) atomicMax(ctr + kCtrEnd0, e0 + 7u);
}
__device__ __forceinline__ void note_written(uint32_t *ctr, uint32_t a, uint32_t z) {
  atomicMin(ctr + kCtrLo, a);
  atomicMax(ctr + kCtrHi, z);
}

// the only launch that writes the pool: one thread per item of the whole plan
__global__ __launch_bounds__(256) void write_kernel(uint8_t *pool, uint32_t start1, const Item *items, uint32_t n, int value, uint32_t *ctr) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const Item it = items[i];
  const uint32_t dec = decision(it), vb = it.bits & kValueMask, ptr = it.ptr;
  const bool is_new = it.bits & kNew;
  const uint32_t pptr = items[it.parent].ptr;
  if (is_new) {
    uint8_t rec[7] = {(uint8_t)vb, 0, 0, 0, 0, 0, 0};
    if (dec == kSetValue || (dec == kSubdivide && value != 0)) rec[0] = (uint8_t)value;
    if (it.bits & kShort) {
      const uint32_t normal = (it.bits >> kNormalShift) & 0x3ffu;
      pool[ptr] = rec[0]; pool[ptr + 1] = (uint8_t)normal; pool[ptr + 2] = (uint8_t)(normal >> 8);
    } else {
      if (dec == kSubdivide) {
        const uint32_t rel = items[it.first_child].ptr - ptr;
        uint32_t mask = (items[it.first_child].bits & kShort) ? 0x5555u : 0xaaaau;
        for (uint32_t c = 0; c < 8u; c++)
          if (decision(items[it.first_child + c]) == kSubdivide) mask &= ~(3u << (2u * c));
        rec[1] = (uint8_t)(rel >> 24); rec[2] = (uint8_t)(rel >> 16); rec[3] = (uint8_t)(rel >> 8); rec[4] = (uint8_t)rel;
        rec[5] = (uint8_t)(mask >> 8); rec[6] = (uint8_t)mask;
      }
      for (int k = 0; k < 7; k++) pool[ptr + k] = rec[k];
    }
  } else if (dec == kSetValue) {
    pool[ptr] = (uint8_t)value;
    note_written(ctr, ptr, ptr + 1u);
  } else if (dec == kSubdivide) {
    const uint32_t rel = items[it.first_child].ptr - ptr;
    uint32_t mask = (items[it.first_child].bits & kShort) ? 0x5555u : 0xaaaau;
    for (uint32_t c = 0; c < 8u; c++)
      if (decision(items[it.first_child + c]) == kSubdivide) mask &= ~(3u << (2u * c));
    if (value != 0) pool[ptr] = (uint8_t)value;
    pool[ptr + 1] = (uint8_t)(rel >> 24); pool[ptr + 2] = (uint8_t)(rel >> 16); pool[ptr + 3] = (uint8_t)(rel >> 8); pool[ptr + 4] = (uint8_t)rel;
    pool[ptr + 5] = (uint8_t)(mask >> 8); pool[ptr + 6] = (uint8_t)mask;
    note_written(ctr, value != 0 ? ptr : ptr + 1u, ptr + 7u);
  } else if (dec == kFill) {
    uint32_t cptr[8], ctag[8];
    // (decide_kernel has checked these bytes; checked again, so that a pool with shared subtrees, where another thread may
    // have rewritten them by now, still stays in bounds)
    bool inside;
    if (i == 0u) {
      // The root is its own parent, child number 0: the reference re-tags that child to a 7-byte leaf in the root's mask
      // BEFORE it walks the root's children (Octree.java:797-808), so the walk lays them out by the patched mask -- where
      // child 0 was a 3-byte or 1-byte record, the marks land behind the other children's value bytes.  Only value bytes
      // are written, so only they have to lie below start1.
      const uint32_t mask = (((((uint32_t)pool[5] << 8) | (uint32_t)pool[6]) & ~3u) | 2u);
      inside = children_at(pool, start1, ptr, mask, false, cptr, ctag);
      pool[5] = (uint8_t)(mask >> 8); pool[6] = (uint8_t)mask;
      note_written(ctr, 5u, 7u);
    } else {
      inside = children_of(pool, start1, ptr, cptr, ctag);
    }
    pool[ptr] = (uint8_t)value;
    note_written(ctr, ptr, ptr + 1u);
    for (uint32_t c = 0; inside && c < 8u; c++) {       // markNodeAsDirty
      pool[cptr[c]] = kDeleteValue;
      note_written(ctr, cptr[c], cptr[c] + 1u);
    }
  } else if (dec == kRecurse) {
    uint32_t mask = ((uint32_t)pool[ptr + 5] << 8) | (uint32_t)pool[ptr + 6];
    bool changed = false;
    for (uint32_t c = 0; c < 8u; c++) {
      const uint32_t cd = decision(items[it.first_child + c]);
      if (cd == kSubdivide) { mask &= ~(3u << (2u * c)); changed = true; }
      else if (cd == kFill) { mask = (mask & ~(3u << (2u * c))) | (2u << (2u * c)); changed = true; }
    }
    if (changed) {
      pool[ptr + 5] = (uint8_t)(mask >> 8); pool[ptr + 6] = (uint8_t)mask;
      note_written(ctr, ptr + 5u, ptr + 7u);
    }
  }
  if (dec == kSetValue) note_bounds(ctr, start1, ptr, ptr);
  else if (dec == kSubdivide) {
    if (value != 0) note_bounds(ctr, start1, ptr, ptr);
    note_bounds(ctr, start1, pptr, ptr);
    atomicAdd(ctr + kCtrSubdivided, 1u);
  } else if (dec == kFill) note_bounds(ctr, start1, pptr, ptr);
}

// ---------------------------------------------------------------------------------------------------------------------
struct State {
  Item *items = nullptr;
  uint32_t cap = 0;
  uint32_t *ctr = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // svo_brush_info: what the last stroke did
  uint64_t strokes = 0, visited = 0, subdivided = 0, lo = 0, hi = 0;
  float gpu_ms = 0.0f;
};
constexpr uint32_t kFirstCap = 1u << 18, kLastCap = 1u << 23;

inline void free_state(State &b) {
  if (b.items) (void)hipFree(b.items);
  if (b.ctr) (void)hipFree(b.ctr);
  if (b.e0) (void)hipEventDestroy(b.e0);
  if (b.e1) (void)hipEventDestroy(b.e1);
  b = State();
}

struct Plan {
  uint32_t flags = 0;          // kFlag*
  uint32_t items = 0;          // visited nodes
  uint32_t appended = 0;       // bytes behind the old end
};

// PLAN: reads the pool, writes the work items only.
inline hipError_t plan(State &b, const uint8_t *d_pool, uint32_t pool_len, const Sdf &s, int value, int world_size, int max_lod,
                       hipStream_t stream, Plan &out) {
  hipError_t e;
  uint32_t h[kCtrWords] = {1u, 0u, pool_len, 0u, 0xffffffffu, 0u, 0u, 0u};
  if ((e = hipMemcpyAsync(b.ctr, h, sizeof h, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
  uint8_t rootv = 0;
  if ((e = hipMemcpyAsync(&rootv, d_pool, 1, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  Item root{};
  root.bits = rootv;     // the root: not a leaf, child 0 of itself
  root.base = pool_len;
  if ((e = hipMemcpyAsync(b.items, &root, sizeof root, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
  uint32_t level_lo[kMaxLevels + 1];
  int levels = 0;
  uint32_t lo = 0, hi = 1;
  int size = world_size;
  while (lo < hi && levels < kMaxLevels) {
    level_lo[levels] = lo;
    const uint32_t n = hi - lo;
    if (size > 0) {
      // lanes per node: the rows of a node of this size, at most a wave; rows per wave: 64 per lane at least, 32768 chunks at most
      const uint64_t rows = (uint64_t)size * (uint64_t)size;
      uint32_t lanes = 1;
      while (lanes < 64u && lanes < rows) lanes *= 2u;
      uint32_t chunks = (uint32_t)std::min<uint64_t>(32768u, (rows + 64u * lanes - 1u) / (64u * lanes));
      const uint32_t iters = (uint32_t)((rows + (uint64_t)lanes * chunks - 1u) / ((uint64_t)lanes * chunks));
      const uint32_t per_wave = 64u / lanes;
      hipLaunchKernelGGL(march_kernel, dim3((n + per_wave - 1u) / per_wave, chunks), dim3(64), 0, stream, b.items, lo, n, size, s, lanes, iters);
    }
    hipLaunchKernelGGL(decide_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_pool, pool_len, b.items, lo, n, size, levels, value, max_lod,
                       b.cap, b.ctr, s);
    if ((e = hipMemcpyAsync(h, b.ctr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    levels++;
    if (h[kCtrFlags]) { out.flags = h[kCtrFlags]; return hipSuccess; }
    lo = hi; hi = h[kCtrItems];
    size /= 2;
  }
  if (lo < hi) { out.flags = kFlagBounds; return hipSuccess; }   // (cannot happen: size 0 has no rows)
  level_lo[levels] = hi;
  for (int l = levels - 1; l >= 0; l--) {
    const uint32_t n = level_lo[l + 1] - level_lo[l];
    hipLaunchKernelGGL(sum_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, b.items, level_lo[l], n);
  }
  for (int l = 0; l < levels; l++) {
    const uint32_t n = level_lo[l + 1] - level_lo[l];
    hipLaunchKernelGGL(offsets_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, b.items, level_lo[l], n);
  }
  if ((e = hipMemcpyAsync(&root, b.items, sizeof root, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  if ((e = hipGetLastError()) != hipSuccess) return e;
  out.items = hi;
  out.appended = root.sub_bytes;
  return hipSuccess;
}

}  // namespace brush
}  // namespace svo
