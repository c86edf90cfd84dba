// Prints what persist_plan (svo-raytracer_amd/csrc/svo_persist_plan.h) decides about the dense shading pass for a fixed list of
// launches, one line per case and setting of PersistSettings::dense_mode:
//   <name> dense_mode=<0|1> dense=.. ray_records=.. old=<every field the plan had before the pass, joined by commas>
// Host code only: built with a plain C++ compiler and run by tests/test_persist_plan_dense.py, which holds the expected values.
#include "svo_persist_plan.h"

#include <cstdio>
#include <cstring>

using namespace svo;

static Frame batch(int w, int h, int n) {
  Frame f;
  memset(&f, 0, sizeof f);
  f.width = w; f.height = h; f.y1 = h; f.row_step = 1;
  f.tiles_x = (w + 7) / 8; f.tiles_y = (h + 7) / 8; f.ntiles = f.tiles_x * f.tiles_y;
  f.render_mode = 0; f.bounces = 2; f.spp = 1; f.batch = n; f.seq = 1;
  f.frame_stride = (uint32_t)(w * h);
  return f;
}

static void show(const char *name, PersistSettings s, const Frame &f, LaunchShape shape, bool table) {
  PersistLimits lim;
  lim.known = true; lim.cus = 256; lim.max_per_cu = 20; lim.max_per_cu_desc = 24;
  const size_t out_npix = (size_t)f.width * (size_t)f.height * (size_t)(f.batch > 1 ? f.batch : 1);
  for (int mode = 0; mode < 2; mode++) {
    s.dense_mode = mode;
    const PersistPlan p = persist_plan(s, lim, f, shape, 0, table, false, false, out_npix);
    printf("%s dense_mode=%d dense=%d ray_records=%zu old=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%u,%u,%u,%u,%zu,%zu,%zu,%zu,%zu,%zu\n", name, mode,
           (int)p.dense, p.ray_records, (int)p.invalid, (int)p.spare, p.per_cu, p.full_blocks, p.blocks, p.thresh_num, p.fold, p.launches,
           (int)p.sequence, (int)p.resolve, (int)p.span, p.slot_frames, (int)p.tables, (int)p.cache, p.mg_rows[0], p.mg_rows[1], p.mg_tpf[0],
           p.mg_tpf[1], (size_t)p.rows_per_band, p.npix, p.facc_floats, p.prim_waves, p.rc_floats, p.kept_records);
  }
}

int main() {
  const PersistSettings def;
  const Frame b4 = batch(64, 64, 4);
  show("batch4", def, b4, kRing, true);
  { Frame f = b4; f.bounces = 3; show("batch4_3bounces", def, f, kRing, true); }
  { Frame f = b4; f.bounces = 5; show("batch4_5bounces", def, f, kRing, true); }
  { Frame f = b4; f.write_hits = 1; show("batch4_hits", def, f, kRing, true); }
  { PersistSettings s; s.table_mode = 0; show("batch4_notables", s, b4, kRing, true); }
  { PersistSettings s; s.kept_mode = 0; show("batch4_nocache", s, b4, kRing, true); }
  { Frame f = b4; f.mirror_mask = 8u; show("batch4_mirror", def, f, kRing, true); }
  // rows that are no multiple of a tile: the records cover whole tile rows, like the cache's
  show("batch7_76x44", def, batch(76, 44, 7), kRing, true);
  show("hd_batch4", def, batch(1920, 1080, 4), kRing, true);
  show("single", def, batch(64, 64, 1), kPlain, true);
  return 0;
}
