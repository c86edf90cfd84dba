// Walks every slot of every band of a fixed list of launches through the pure half of the persistent kernels' draw
// (svo-raytracer_amd/csrc/svo_persist_plan.h: band_of, slot_tile, slot_pixel) and prints, one line per case:
//   <name> slots=<slots walked> drawn=<(frame, sample, pixel) triples decoded> want=<triples of the set> bad=<violations> ...
// The set a launch must produce is written down here from its definition -- {frames} x {samples} x {pixels of the launch's rows
// inside the frame}, each once, at output index fi * frame_stride + output row * width + px -- not from the functions under test.
// Host code only: built with a plain C++ compiler and run by tests/test_persist_draw.py.
#include "svo_persist_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

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

// real_division: the reciprocals zeroed, as udiv_magic returns them for a dividend past what they are exact for
static void walk(const char *name, const PersistSettings &set, const Frame &f, int group, bool real_division) {
  PersistLimits lim;
  lim.known = true; lim.cus = 256; lim.max_per_cu = 20; lim.max_per_cu_desc = 24;
  PersistPlan p = persist_plan(set, lim, f, kRing, 0, true, false, false, (size_t)f.width * (size_t)f.height * (size_t)f.batch);
  const int magics = (p.mg_rows[0] != 0) + (p.mg_rows[1] != 0) + (p.mg_tpf[0] != 0) + (p.mg_tpf[1] != 0);
  if (real_division) p.mg_rows[0] = p.mg_rows[1] = p.mg_tpf[0] = p.mg_tpf[1] = 0u;
  const int frames = p.span ? 1 : f.batch, fold = p.fold;

  // the set: how often each (frame, sample, px, py) must turn up, and where its pixel goes
  const size_t plane = (size_t)f.width * (size_t)f.height;
  std::vector<int> want(plane * frames * fold, 0), got(plane * frames * fold, 0);
  std::vector<uint32_t> index(plane, 0u);
  unsigned long long n_want = 0;
  for (int ty = 0; ty < f.tiles_y; ty++)
    for (int ly = 0; ly < 8; ly++) {
      const int py = f.y0 + ty * 8 * f.row_step + ly;
      if (py >= f.y1 || py >= f.height) continue;
      for (int px = 0; px < f.width; px++) {
        index[(size_t)py * f.width + px] = (uint32_t)((f.out_y0 + ty * 8 + ly) * f.width + px);
        for (int k = 0; k < frames * fold; k++) { want[(size_t)k * plane + (size_t)py * f.width + px] = 1; n_want++; }
      }
    }

  unsigned long long slots = 0, drawn = 0, bad = 0;
  int full = 0, part = 0, empty = 0, cut_x = 0, cut_y1 = 0, cut_h = 0;
  for (int reverse = 0; reverse < 2; reverse++)
    for (uint32_t band = 0; band < 8u; band++) {
      const Band b = band_of(band, p.rows_per_band, f.tiles_x, f.tiles_y, f.batch, fold, p.span);
      if (reverse == 0) { full += b.rows == p.rows_per_band; part += b.rows > 0 && b.rows < p.rows_per_band; empty += b.rows == 0; }
      if (b.total != (uint32_t)(b.rows * f.tiles_x * 64 * frames * fold)) bad++;
      for (uint32_t slot = 0; slot < b.total; slot++) {
        const SlotTile s = slot_tile(b, slot, p.rows_per_band, f.tiles_x, reverse, p.mg_rows, p.mg_tpf, f.batch, fold, group, p.span);
        const SlotTile m = slot_tile(b, slot, p.rows_per_band, f.tiles_x, 1 - reverse, p.mg_rows, p.mg_tpf, f.batch, fold, group, p.span);
        // the other direction: the same frame, sample, tile row and pixel of the tile, the mirrored tile column
        if (m.fi != s.fi || m.si != s.si || m.tile_y != s.tile_y || m.l != s.l || m.tile_x != f.tiles_x - 1 - s.tile_x) bad++;
        if (s.fi >= (uint32_t)frames || s.si >= (uint32_t)fold || s.tile_x < 0 || s.tile_x >= f.tiles_x || s.tile_y < b.first_row ||
            s.tile_y >= b.first_row + b.rows || s.tile_y >= f.tiles_y || s.l != (slot & 63u)) { bad++; continue; }
        const SlotPixel q = slot_pixel(f, s);
        if (reverse == 0) { slots++; cut_x += q.px >= f.width; cut_y1 += q.py >= f.y1; cut_h += q.py >= f.height; }
        if (q.inside != (q.px < f.width && q.py < f.y1 && q.py < f.height)) bad++;
        if (!q.inside) continue;
        if (q.px < 0 || q.py < 0) { bad++; continue; }
        const size_t at = (size_t)q.py * f.width + q.px;
        if (q.pix != s.fi * f.frame_stride + index[at]) bad++;
        if (reverse == 0) { got[((size_t)s.fi * fold + s.si) * plane + at]++; drawn++; }
        else got[((size_t)s.fi * fold + s.si) * plane + at] += 2;
      }
    }
  // each triple once in either direction: 1 + 2
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != 3 * want[i]) bad++;
  printf("%s slots=%llu drawn=%llu want=%llu bad=%llu span=%d fold=%d rows_per_band=%d full=%d part=%d empty=%d cut_x=%d cut_y1=%d cut_h=%d magics=%d\n",
         name, slots, drawn, n_want, bad, (int)p.span, fold, p.rows_per_band, full, part, empty, cut_x, cut_y1, cut_h, magics);
}

int main() {
  const PersistSettings def;
  PersistSettings nospan;
  nospan.span_mode = 0;
  walk("one_tile", def, frame(8, 8), 8, false);
  const Frame odd = frame(21, 130);   // 3 x 17 tiles: bands of 3 tile rows, the last of 2, two empty; the right column cut
  walk("odd", def, odd, 8, false);
  walk("odd_real_division", def, odd, 8, true);
  {
    Frame f = odd;   // every other tile row from pixel row 8 on, four of them, the last cut by y1; packed from output row 5
    f.y0 = 8; f.row_step = 2; f.tiles_y = 4; f.ntiles = f.tiles_x * f.tiles_y; f.y1 = 60; f.out_y0 = 5;
    walk("stripe", def, f, 8, false);
  }
  {
    Frame f = frame(21, 140);   // 18 tile rows: the last of them hangs over the frame's height, not over y1
    f.y1 = 1000;
    walk("cut_by_height", def, f, 8, false);
  }
  { Frame f = odd; f.batch = 3; walk("batch3_frame_pixel", nospan, f, 8, false); }
  { Frame f = odd; f.batch = 3; walk("batch3_pixel", def, f, 8, false); }
  { Frame f = frame(72, 8); f.spp = 3; walk("fold3", def, f, 8, false); }   // one band of 9 tiles: a group of 8 and a group of 1
  { Frame f = odd; f.spp = 3; f.batch = 2; walk("fold3_batch2", def, f, 2, false); }
  return 0;
}
