// The pure half of the dense pass's ray list (svo-raytracer_amd/csrc/svo_persist_plan.h: ray_region, ray_run_reserve,
// ray_run_take), run on the host.  Prints, one line per case:
//   run fill=<n> waves=<w> lanes=<pattern> handed=<entries handed out> twice=<handed out more than once> beyond=<at or past the fill>
//       missed=<below the fill and never handed out> reservations=<atomics on the cursor>
//   region <w>x<h>x<frames> records=<plan.ray_records> dense=<0|1> bands=<first:room,...>
//   const chunk=<kChunk> bytes=<kRayListBytes> ...
// Host code only: built with a plain C++ compiler (and once with -fsanitize=address,undefined) and run by
// tests/test_ray_list_plan.py, which holds the expected values.
#include "svo_persist_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace svo;

// `waves` waves draw from one band of `fill` entries, taking turns in a fixed schedule: wave w's k-th draw has
// 1 + (w * 7 + k * step) % 64 idle lanes, like persist_runs_kernel's refill: reserve when the run is used up, move on when it was the
// band's last.  A wave that has left the band stops.
static void run_case(uint32_t fill, int waves, int step) {
  std::vector<uint32_t> handed(fill + 4u * kChunk + 64u, 0u);
  struct Wave { RayRun run; bool gone; uint32_t draws; };
  std::vector<Wave> ws((size_t)waves);
  for (auto &w : ws) { w.run.cur = 0u; w.run.end = 0u; w.run.last = false; w.gone = false; w.draws = 0u; }
  uint32_t cursor = 0u, reservations = 0u, out = 0u, twice = 0u, beyond = 0u;
  for (int left = waves; left > 0;) {
    for (int i = 0; i < waves; i++) {
      Wave &w = ws[(size_t)i];
      if (w.gone) continue;
      const uint32_t idle = 1u + (uint32_t)(i * 7 + (int)w.draws * step) % 64u;
      w.draws++;
      uint32_t want = idle;
      while (want > 0u) {   // one round: runs follow one another while the band has entries
        if (w.run.cur == w.run.end) {
          if (w.run.last) { w.gone = true; left--; break; }
          const uint32_t base = cursor;
          cursor += kChunk;
          reservations++;
          w.run = ray_run_reserve(base, fill);
          continue;
        }
        const uint32_t at = w.run.cur, n = ray_run_take(w.run, want);
        for (uint32_t r = 0; r < n; r++) {
          const uint32_t e = at + r;
          if (e >= fill) beyond++;
          if (e < handed.size() && handed[e]++ != 0u) twice++;
          out++;
        }
        want -= n;
      }
    }
  }
  uint32_t missed = 0u;
  for (uint32_t e = 0; e < fill; e++) missed += handed[e] == 0u ? 1u : 0u;
  printf("run fill=%u waves=%d step=%d handed=%u twice=%u beyond=%u missed=%u reservations=%u\n", fill, waves, step, out, twice, beyond, missed, reservations);
}

static void region_case(int w, int h, int frames) {
  Frame f;
  memset(&f, 0, sizeof f);
  f.width = w; f.height = h; f.y1 = h; f.row_step = 1;
  f.tiles_x = (w + 7) / 8; f.tiles_y = (h + 7) / 8; f.ntiles = f.tiles_x * f.tiles_y;
  f.render_mode = 0; f.bounces = 2; f.spp = 1; f.batch = frames; f.seq = 1;
  f.frame_stride = (uint32_t)(w * h);
  PersistSettings s;
  s.list_mode = 1;
  PersistLimits lim;
  lim.known = true; lim.cus = 256; lim.max_per_cu = 20; lim.max_per_cu_desc = 24;
  const PersistPlan p = persist_plan(s, lim, f, kRing, 0, true, false, false, (size_t)w * (size_t)h * (size_t)frames);
  printf("region %dx%dx%d records=%zu dense=%d list=%d rows_per_band=%d bands=", w, h, frames, p.ray_records, (int)p.dense, (int)p.list, p.rows_per_band);
  for (uint32_t b = 0; b < 8u; b++) {
    const RayRegion r = ray_region(b, p.rows_per_band, f.tiles_y, f.width, frames);
    printf("%s%u:%u", b ? "," : "", r.first, r.room);
  }
  printf("\n");
}

int main() {
  printf("const chunk=%u bytes=%zu slot_bytes=%zu index_bits=%u max_frames=%d list_default=%d\n", kChunk, kRayListBytes, kRayBytes, kRayIndexBits, kRayMaxFrames, (int)PersistSettings().list_mode);
  const uint32_t fills[] = {0u, 1u, kChunk - 1u, kChunk, kChunk + 1u, 3000u, 7777u};
  for (uint32_t fill : fills)
    for (int waves : {1, 3, 10})
      for (int step : {1, 13, 63}) run_case(fill, waves, step);

  for (int frames : {2, 4, 7}) {
    region_case(76, 44, frames);
    region_case(76, 8, frames);
    region_case(1920, 1080, frames);
  }
  // what does not fit a record's last word takes no dense pass: 256 frames, or more than 2^24 pixels
  region_case(64, 64, 255);
  region_case(64, 64, 256);
  region_case(4096, 4096, 2);
  region_case(4104, 4096, 2);
  {   // without lists the same launch keeps its dense pass: a record per (frame, pixel) needs no index bits
    Frame f;
    memset(&f, 0, sizeof f);
    f.width = 64; f.height = 64; f.y1 = 64; f.row_step = 1; f.tiles_x = 8; f.tiles_y = 8; f.ntiles = 64;
    f.bounces = 2; f.spp = 1; f.batch = 256; f.seq = 1; f.frame_stride = 64u * 64u;
    PersistSettings s;
    s.list_mode = 0;
    PersistLimits lim;
    lim.known = true; lim.cus = 256; lim.max_per_cu = 20; lim.max_per_cu_desc = 24;
    const PersistPlan p = persist_plan(s, lim, f, kRing, 0, true, false, false, (size_t)64 * 64 * 256);
    printf("slots 64x64x256 records=%zu dense=%d list=%d\n", p.ray_records, (int)p.dense, (int)p.list);
  }
  return 0;
}
