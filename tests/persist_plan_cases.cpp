// Prints persist_plan's decisions (svo-raytracer_amd/csrc/svo_persist_plan.h) for a fixed list of launches, one line per case:
//   <name> key=value ...
// and checks every reciprocal the plan hands the kernels against a real division.  Host code only: built with a plain C++
// compiler and run by tests/test_persist_plan.py, which holds the expected values.
#include "svo_persist_plan.h"

#include <cstdio>
#include <cstring>

using namespace svo;

static Frame frame(int w, int h) {
  Frame f;
  memset(&f, 0, sizeof f);
  f.width = w; f.height = h; f.y1 = h; f.row_step = 1;
  f.tiles_x = (w + 7) / 8; f.tiles_y = (h + 7) / 8; f.ntiles = f.tiles_x * f.tiles_y;
  f.render_mode = 0; f.bounces = 2; f.spp = 1; f.batch = 1; f.seq = 1;
  f.frame_stride = (uint32_t)(w * h);
  return f;
}

static Frame batch(int w, int h, int n) {
  Frame f = frame(w, h);
  f.batch = n;
  return f;
}

struct Walk { bool table, cams; };
static const Walk kTable = {true, false}, kRecords = {false, false}, kTableCams = {true, true};

// (n m) >> 32 == n / d for every n up to n_max, for a reciprocal the plan did not decline (m != 0)
static void check_magic(uint32_t d, uint64_t n_max, uint32_t m, unsigned long long &checked, unsigned long long &bad) {
  if (m == 0u) return;
  for (uint64_t n = 0; n <= n_max; n++) {
    checked++;
    if ((uint32_t)((n * (uint64_t)m) >> 32) != (uint32_t)(n / d)) bad++;
  }
}

static void show(const char *name, const PersistSettings &s, const Frame &f, LaunchShape shape, int sets, Walk w) {
  PersistLimits lim;
  lim.known = true; lim.cus = 256; lim.max_per_cu = 20; lim.max_per_cu_desc = 24;
  const size_t out_npix = (size_t)f.width * (size_t)f.height * (size_t)(f.batch > 1 ? f.batch : 1);
  const PersistPlan p = persist_plan(s, lim, f, shape, sets, w.table, w.cams, false, out_npix);
  // the divisors and the largest dividends, as the kernel forms them: a band's tile rows (dividend: a tile of the band) and its
  // tile slots per frame (dividend: a tile slot of the band over the frames its slots are counted over), full band / last band
  const int rows = (f.tiles_y + 7) / 8, last = rows > 0 ? f.tiles_y % rows : 0;
  const int frames = p.span ? 1 : (f.batch > 1 ? f.batch : 1);
  unsigned long long checked = 0, bad = 0;
  check_magic((uint32_t)rows, (uint64_t)rows * f.tiles_x, p.mg_rows[0], checked, bad);
  check_magic((uint32_t)last, (uint64_t)last * f.tiles_x, p.mg_rows[1], checked, bad);
  check_magic((uint32_t)(rows * f.tiles_x * p.fold), (uint64_t)frames * (uint64_t)(rows * f.tiles_x * p.fold), p.mg_tpf[0], checked, bad);
  check_magic((uint32_t)(last * f.tiles_x * p.fold), (uint64_t)frames * (uint64_t)(last * f.tiles_x * p.fold), p.mg_tpf[1], checked, bad);
  printf("%s invalid=%d per_cu=%d blocks=%d thresh=%d fold=%d launches=%d sequence=%d resolve=%d span=%d slot_frames=%d tables=%d cache=%d "
         "rows_per_band=%d facc_floats=%zu prim_waves=%zu rc_floats=%zu kept_records=%zu magics=%d magic_checked=%llu magic_bad=%llu\n",
         name, (int)p.invalid, p.per_cu, p.blocks, p.thresh_num, p.fold, p.launches, (int)p.sequence, (int)p.resolve, (int)p.span,
         p.slot_frames, (int)p.tables, (int)p.cache, p.rows_per_band, p.facc_floats, p.prim_waves, p.rc_floats, p.kept_records,
         (p.mg_rows[0] != 0) + (p.mg_rows[1] != 0) + (p.mg_tpf[0] != 0) + (p.mg_tpf[1] != 0), checked, bad);
}

int main() {
  const PersistSettings def;
  const Frame hd = frame(1920, 1080);
  show("hd_plain", def, hd, kPlain, 0, kTable);
  show("hd_ring", def, hd, kRing, 0, kTable);
  show("hd_overlap2", def, hd, kOverlap, 2, kTable);
  show("hd_overlap3", def, hd, kOverlap, 3, kTable);
  show("hd_overlap4", def, hd, kOverlap, 4, kTable);
  show("hd_overlap5", def, hd, kOverlap, 5, kTable);
  show("hd_records", def, hd, kPlain, 0, kRecords);
  {
    PersistSettings s;   // svo_set_tuning(3, 11)
    s.waves_per_cu = 3; s.thresh_num = 11;
    show("hd_tuned_plain", s, hd, kPlain, 0, kTable);
    show("hd_tuned_ring", s, hd, kRing, 0, kTable);
    show("hd_tuned_overlap4", s, hd, kOverlap, 4, kTable);
    show("hd_tuned_records", s, hd, kPlain, 0, kRecords);
  }
  {
    PersistSettings s;   // two reserved CUs on each of the 8 XCDs
    s.cus_reserved = 16;
    show("hd_reserved_plain", s, hd, kPlain, 0, kTable);
    show("hd_reserved_ring", s, hd, kRing, 0, kTable);
  }
  show("tiny", def, frame(8, 8), kPlain, 0, kTable);

  const Frame b4 = batch(64, 64, 4);
  show("batch4", def, b4, kRing, 0, kTable);
  { Frame f = b4; f.write_hits = 1; show("batch4_hits", def, f, kRing, 0, kTable); }
  { PersistSettings s; s.table_mode = 0; show("batch4_notables", s, b4, kRing, 0, kTable); }
  { PersistSettings s; s.kept_mode = 0; show("batch4_nocache", s, b4, kRing, 0, kTable); }
  show("batch4_cams", def, b4, kRing, 0, kTableCams);
  { Frame f = b4; f.bounces = 1; show("batch4_1bounce", def, f, kRing, 0, kTable); }
  { Frame f = b4; f.use_beam = 1; show("batch4_beam", def, f, kRing, 0, kTable); }
  { Frame f = b4; f.spp = 4; show("batch4_spp4", def, f, kRing, 0, kTable); }
  { Frame f = b4; f.render_mode = 2; show("batch4_mode2", def, f, kRing, 0, kTable); }
  show("batch4_records", def, b4, kRing, 0, kRecords);
  { PersistSettings s; s.span_mode = 0; show("batch4_nospan", s, b4, kRing, 0, kTable); }

  { Frame f = frame(64, 64); f.spp = 4; show("spp4", def, f, kPlain, 0, kTable); }
  { Frame f = frame(64, 64); f.progressive = 1; f.seq = 3; show("seq3", def, f, kPlain, 0, kTable); }
  { Frame f = frame(64, 64); f.progressive = 1; f.seq = 3; f.spp = 2; show("seq3_spp2", def, f, kPlain, 0, kTable); }
  { Frame f = frame(3840, 2160); f.spp = 64; show("uhd_spp64", def, f, kPlain, 0, kTable); }
  return 0;
}
