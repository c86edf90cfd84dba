// svo_compact.hip.h -- the device pool rewritten as exactly its reachable records, in the builder's order (svo_pool_compact,
// include/svo_hip.h).  Included by svo_hip.hip.
//
// The brush (svo_brush.hip.h) only ever appends, like Octree.useSDFBrush: a subdivision writes its children block at the pool's
// end, a fill re-tags a node as a leaf and leaves its former subtree where it was, unreachable.  The reference has no answer
// (Octree.getSubtreeRange is a stub).  Here:
//   * reachable: the root record at offset 0 (always interior) and the eight children of every reachable record whose tag in
//     its parent's mask is 0 -- by tag, not by value: an interior node of value 0 keeps its subtree, a tag-2 leaf's stale child
//     pointer is not followed;
//   * order: svo_build.hip.h step 3 -- the root, its children block, then the subtrees of the block's tag-0 children in child
//     order, each laid out the same way: the block of the n-th interior node in depth-first preorder is the n-th block;
//   * bytes: every record verbatim (a tag-2 leaf keeps bytes 1..6, SURVEY Q5 shades from them), only the big-endian relative
//     child pointer of the interior records, the root's included, is recomputed.  No gaps, no padding.
// Plan first, write once, as the brush and the builder do.  A level is the list of the nodes that own a children block, in
// depth-first order.  Top-down, one launch per level (descend_kernel): a thread per (node, child) takes the tag-0 children,
// reads their pointer and mask, checks that the block they name lies inside the pool BEFORE anything reads it, and stores the
// node of the next level at the place the builder's exclusive scan gave it.  Bottom-up (sum_kernel): bytes of every subtree.
// Top-down (place_kernel): the new offset of every block.  One launch per level of write_kernel copies the records into a
// second buffer and writes the pointers; the caller swaps the buffers.  A plan that fails -- a block outside the pool, more
// levels than the walk supports, too many nodes, a result of 2^31 bytes -- has written nothing but its own lists.
// A block that two interior records share is reached twice and copied twice: the result is a tree.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "svo_build.hip.h"
#include "svo_device.h"

namespace svo {
namespace compact {

// Levels of block-owning nodes a pool may have: the ray walk pushes once per descent and its stack has kStackLevels entries,
// so it stands on kStackLevels + 1 levels of parents (depth 0..12, the reference's MAX_DEPTH).  A cycle in a mangled pool
// unrolls into ever more levels and ends here.
constexpr int kMaxLevels = kStackLevels + 1;
static_assert(kMaxLevels == kMaxDepth, "the level bound is the walker's depth");
// Nodes of all levels together: kNodeBytes of list each, 2.5 GiB at the cap (a tree of 2^31 bytes has fewer than 2^28 blocks;
// only a pool whose blocks are shared many times over gets near)
constexpr uint32_t kMaxNodes = 1u << 27;
constexpr uint32_t kNodeBytes = 20;

struct Level {
  uint32_t *blk = nullptr;     // the node's children block in the old pool
  uint16_t *mask = nullptr;    // its children's tags
  uint8_t *bytes = nullptr;    // bytes of the block
  uint8_t *em = nullptr;       // children of tag 0: they own a block themselves (0 for a node whose block lies outside the pool)
  uint32_t *first = nullptr;   // index of the first such child in the next level
  uint32_t *sub = nullptr;     // bytes of the subtree below the node: its block + its children's subtrees (saturating)
  uint32_t *start = nullptr;   // the block in the new pool
  uint32_t count = 0;
};

__host__ __device__ inline uint32_t block_bytes(uint32_t mask) {
  const uint32_t lo = mask & 0x5555u, both = lo & (mask >> 1);
  return 56u - 4u * (uint32_t)__builtin_popcount(lo) - 2u * (uint32_t)__builtin_popcount(both);
}
__host__ __device__ inline uint32_t interior_children(uint32_t mask) {
  uint32_t em = 0;
  for (uint32_t c = 0; c < 8u; c++)
    if (((mask >> (2u * c)) & 3u) == 0u) em |= 1u << c;
  return em;
}
// byte offset of child n inside a block (svo_build.hip.h::emit_kernel)
__device__ __forceinline__ uint32_t child_offset(uint32_t mask, uint32_t n) {
  const uint32_t below = (1u << (2u * n)) - 1u, lo = mask & 0x5555u & below, both = lo & (mask >> 1);
  return 7u * n - 4u * (uint32_t)__builtin_popcount(lo) - 2u * (uint32_t)__builtin_popcount(both);
}
__host__ __device__ inline bool block_inside(long long blk, uint32_t bytes, uint32_t pool_len) {
  return blk >= 0 && blk + (long long)bytes <= (long long)pool_len;
}

// the tag-0 children of level `p` become the nodes of level `c`: thread = (node, child)
__global__ __launch_bounds__(256) void descend_kernel(const uint8_t *pool, uint32_t pool_len, const Level p, const Level c, uint32_t *bad) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = t >> 3, n = t & 7u;
  if (i >= p.count) return;
  const uint32_t em = p.em[i];
  if (!((em >> n) & 1u)) return;
  const uint8_t *rec = pool + p.blk[i] + child_offset(p.mask[i], n);   // inside the pool: the parent's block was checked
  const int cp = (int)(((uint32_t)rec[1] << 24) | ((uint32_t)rec[2] << 16) | ((uint32_t)rec[3] << 8) | (uint32_t)rec[4]);
  const uint32_t mask = ((uint32_t)rec[5] << 8) | (uint32_t)rec[6], bytes = block_bytes(mask);
  const long long blk = (long long)(rec - pool) + (long long)cp;
  const bool inside = block_inside(blk, bytes, pool_len);
  if (!inside) atomicOr(bad, 1u);
  const uint32_t j = p.first[i] + (uint32_t)__builtin_popcount(em & ((1u << n) - 1u));
  c.blk[j] = inside ? (uint32_t)blk : 0u;
  c.mask[j] = (uint16_t)mask;
  c.bytes[j] = (uint8_t)bytes;
  c.em[j] = inside ? (uint8_t)interior_children(mask) : (uint8_t)0;
}

// bottom-up: 0xffffffff says "too large" whatever is added to it (svo_build.hip.h::subtree_kernel)
__global__ __launch_bounds__(256) void sum_kernel(const Level lv, const uint32_t *next_sub) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= lv.count) return;
  uint64_t s = lv.bytes[i];
  const uint32_t k = (uint32_t)__builtin_popcount(lv.em[i]), f = lv.first[i];
  for (uint32_t j = 0; j < k; j++) s += next_sub[f + j];
  lv.sub[i] = s > 0xffffffffull ? 0xffffffffu : (uint32_t)s;
}

// top-down: a block is followed by the subtrees of its children, in order
__global__ __launch_bounds__(256) void place_kernel(const Level lv, const uint32_t *next_sub, uint32_t *next_start) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= lv.count) return;
  const uint32_t k = (uint32_t)__builtin_popcount(lv.em[i]), f = lv.first[i];
  uint32_t at = lv.start[i] + lv.bytes[i];
  for (uint32_t j = 0; j < k; j++) {
    next_start[f + j] = at;
    at += next_sub[f + j];
  }
}

// the only launches that write the new pool: thread = (node, child) copies the child's record; a tag-0 child gets its new
// pointer.  `top`: the level is the root alone, whose own record goes to offset 0.
__global__ __launch_bounds__(256) void write_kernel(const uint8_t *pool, uint8_t *out, const Level lv, const uint32_t *next_start, bool top) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = t >> 3, n = t & 7u;
  if (i >= lv.count) return;
  const uint32_t mask = lv.mask[i], tag = (mask >> (2u * n)) & 3u, off = child_offset(mask, n);
  const uint32_t at = lv.start[i] + off;
  const uint8_t *src = pool + lv.blk[i] + off;
  uint8_t *dst = out + at;
  const uint32_t sz = build::tag_bytes(tag);
  const uint32_t em = lv.em[i];
  dst[0] = src[0];
  if (sz == 3u) {
    dst[1] = src[1]; dst[2] = src[2];
  } else if (sz == 7u) {
    uint32_t p1 = src[1], p2 = src[2], p3 = src[3], p4 = src[4];
    if ((em >> n) & 1u) {
      const uint32_t rel = next_start[lv.first[i] + (uint32_t)__builtin_popcount(em & ((1u << n) - 1u))] - at;
      p1 = rel >> 24; p2 = (rel >> 16) & 255u; p3 = (rel >> 8) & 255u; p4 = rel & 255u;
    }
    dst[1] = (uint8_t)p1; dst[2] = (uint8_t)p2; dst[3] = (uint8_t)p3; dst[4] = (uint8_t)p4;
    dst[5] = src[5]; dst[6] = src[6];
  }
  if (top && t == 0u) {
    const uint32_t rel = lv.start[0];
    out[0] = pool[0];
    out[1] = (uint8_t)(rel >> 24); out[2] = (uint8_t)(rel >> 16); out[3] = (uint8_t)(rel >> 8); out[4] = (uint8_t)rel;
    out[5] = pool[5]; out[6] = pool[6];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct State {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // svo_compact_info: calls so far, and of the last one
  uint64_t calls = 0, records = 0;
  int levels = 0;
  float gpu_ms = 0.0f;
};
inline void free_state(State &s) {
  if (s.e0) (void)hipEventDestroy(s.e0);
  if (s.e1) (void)hipEventDestroy(s.e1);
  s = State();
}

enum Refusal { kDone = 0, kOutside, kTooDeep, kTooManyNodes, kTooLarge };

struct Result {
  Refusal refusal = kDone;
  uint8_t *pool = nullptr;     // device, `pad` zero bytes behind len; the caller owns it
  uint64_t len = 0, cap = 0;   // (len is also set with kTooLarge: what the result would take)
  uint64_t nodes = 0;
  int levels = 0;
};

// Reads d_pool[0, pool_len) (pool_len >= 7) and makes the compacted pool in a buffer of its own.
inline hipError_t run(const uint8_t *d_pool, uint32_t pool_len, uint64_t pad, hipStream_t stream, Result &res) {
  build::Builder B;
  B.stream = stream;
  uint32_t *bad = B.alloc<uint32_t>(1);
  uint8_t root[7] = {};
  if (B.ok()) B.err = hipMemsetAsync(bad, 0, 4, stream);
  if (B.ok()) B.err = hipMemcpyAsync(root, d_pool, 7, hipMemcpyDeviceToHost, stream);
  if (B.ok()) B.err = hipStreamSynchronize(stream);
  if (!B.ok()) { B.release(); return B.err; }
  auto refuse = [&](Refusal r) { B.release(); res.refusal = r; return hipSuccess; };

  auto make_level = [&](uint32_t count) {
    Level L;
    L.count = count;
    L.blk = B.alloc<uint32_t>(count); L.mask = B.alloc<uint16_t>(count); L.bytes = B.alloc<uint8_t>(count); L.em = B.alloc<uint8_t>(count);
    L.first = B.alloc<uint32_t>(count); L.sub = B.alloc<uint32_t>(count); L.start = B.alloc<uint32_t>(count);
    return L;
  };
  // level 0: the root, always interior
  const int root_cp = (int)(((uint32_t)root[1] << 24) | ((uint32_t)root[2] << 16) | ((uint32_t)root[3] << 8) | (uint32_t)root[4]);
  const uint32_t root_mask = ((uint32_t)root[5] << 8) | (uint32_t)root[6], root_bytes = block_bytes(root_mask);
  if (!block_inside((long long)root_cp, root_bytes, pool_len)) return refuse(kOutside);
  std::vector<Level> lv;
  lv.push_back(make_level(1));
  if (B.ok()) {
    const uint32_t blk = (uint32_t)root_cp, start = 7u;
    const uint16_t mk = (uint16_t)root_mask;
    const uint8_t by = (uint8_t)root_bytes, em = (uint8_t)interior_children(root_mask);
    B.err = hipMemcpyAsync(lv[0].blk, &blk, 4, hipMemcpyHostToDevice, stream);
    if (B.ok()) B.err = hipMemcpyAsync(lv[0].mask, &mk, 2, hipMemcpyHostToDevice, stream);
    if (B.ok()) B.err = hipMemcpyAsync(lv[0].bytes, &by, 1, hipMemcpyHostToDevice, stream);
    if (B.ok()) B.err = hipMemcpyAsync(lv[0].em, &em, 1, hipMemcpyHostToDevice, stream);
    if (B.ok()) B.err = hipMemcpyAsync(lv[0].start, &start, 4, hipMemcpyHostToDevice, stream);
    if (B.ok()) B.err = hipStreamSynchronize(stream);   // (the sources are on this frame)
  }
  uint64_t nodes = 1;
  while (B.ok()) {
    const Level L = lv.back();
    uint32_t total = 0;
    B.exclusive_scan<uint8_t, true>(L.em, L.first, L.count, &total);   // (waits for the level: total is on the host)
    if (!B.ok() || total == 0) break;
    if ((int)lv.size() == kMaxLevels) return refuse(kTooDeep);
    nodes += total;
    if (nodes > kMaxNodes) return refuse(kTooManyNodes);
    const Level C = make_level(total);
    if (!B.ok()) break;
    hipLaunchKernelGGL(descend_kernel, dim3((unsigned)(((size_t)L.count * 8 + 255) / 256)), dim3(256), 0, stream, d_pool, pool_len, L, C, bad);
    lv.push_back(C);
  }
  uint32_t h_bad = 0;
  if (B.ok()) B.err = hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, stream);
  if (B.ok()) B.err = hipStreamSynchronize(stream);
  if (!B.ok()) { B.release(); return B.err; }
  if (h_bad) return refuse(kOutside);

  const int levels = (int)lv.size();
  for (int d = levels - 1; d >= 0; d--)
    hipLaunchKernelGGL(sum_kernel, dim3((lv[(size_t)d].count + 255u) / 256u), dim3(256), 0, stream, lv[(size_t)d],
                       d + 1 < levels ? lv[(size_t)d + 1].sub : nullptr);
  uint32_t root_sub = 0;
  if (B.ok()) B.err = hipMemcpyAsync(&root_sub, lv[0].sub, 4, hipMemcpyDeviceToHost, stream);
  if (B.ok()) B.err = hipStreamSynchronize(stream);
  if (!B.ok()) { B.release(); return B.err; }
  const uint64_t total = 7ull + root_sub;
  res.len = total;
  if (total > 0x7fffffffull) return refuse(kTooLarge);   // child pointers are signed 32-bit (Octree.java:162-168)

  for (int d = 0; d + 1 < levels; d++)
    hipLaunchKernelGGL(place_kernel, dim3((lv[(size_t)d].count + 255u) / 256u), dim3(256), 0, stream, lv[(size_t)d], lv[(size_t)d + 1].sub,
                       lv[(size_t)d + 1].start);
  uint8_t *out = nullptr;
  if (B.ok()) B.err = hipMalloc((void **)&out, total + pad);
  if (!B.ok()) { B.release(); return B.err; }
  (void)hipMemsetAsync(out + total, 0, pad, stream);
  for (int d = 0; d < levels; d++)
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)(((size_t)lv[(size_t)d].count * 8 + 255) / 256)), dim3(256), 0, stream, d_pool, out, lv[(size_t)d],
                       d + 1 < levels ? lv[(size_t)d + 1].start : nullptr, d == 0);
  if (B.ok()) B.err = hipStreamSynchronize(stream);
  B.release();
  if (B.err != hipSuccess) {
    (void)hipFree(out);
    return B.err;
  }
  res.pool = out; res.cap = total + pad; res.nodes = nodes; res.levels = levels;
  return hipSuccess;
}

}  // namespace compact
}  // namespace svo
