// rfid_collide.hpp -- the collisions stage of the batched path: behind the statistics of a pass, one rfid_collision per RN16 window
// before the TERMINATED cut-off -- the two handles and the two channels of a slot in which two tags replied at once.  The decoder
// (tag_detection_RN16, tag_decoder_impl.cc:114-142, 237-253) is single-tag by construction: in a collision its 16 bits are a mixture
// of the two replies, and the slots stage can only say that the slot collided.  Decision j is the difference d_j of two adjacent
// half-bit samples; with two synchronous FM0 replies d_j = +-h1 +- h2, and h1 + h2 is the decoder's own h_est.  Squared, the d_j form
// two clusters, one at the known (h1 + h2)^2: a two-means with one centre held separates them, the signed means of the two sets are
// h1 + h2 and h1 - h2, and every d_j is then the nearest of four points.  No counterpart in the reference.  Nothing a pass reports
// changes: the records are a report of their own.
//
// The definition (include/rfid_mi355x.h, rfid_collision) is in binary32, one rounding per operation, every sum in order from 0.0f: a
// record is a function of the input alone.  The shape:
//   lanes    a window is 16 decisions, so a wave takes COL_PACK = 4 windows at a time, one per 16-lane row; lane t of a row gathers
//            the two samples of decision t (the decoder's own gather: y[start + index + 10 t] and 5 behind it, 8-byte loads, the 16
//            lanes of a row 80 bytes apart) and forms d_t and its square w_t.
//   park     (d_t, w_t) go to LDS as one float4, rows COL_STRIDE = 17 float4 apart: 272 bytes, so the four rows start four banks
//            apart and the 16-byte reads of different rows never meet in a bank.  1 088 + 256 bytes per single-wave workgroup.
//   walk     the definition is a chain of seven in-order passes over the 16 points (the farthest square, four rounds of the
//            two-means, the last assignment with the two signed sums, the four-point decisions with the two residual sums): 112
//            dependent steps, not a tree.  EVERY lane of a row walks the chain itself: point j comes as one ds_read_b128 whose address
//            the 16 lanes of the row share (a broadcast), so behind the park no value crosses lanes -- no ballot, no shuffle and no
//            wait on another lane inside the chain -- and all lanes of a row end up holding the whole record.  The lanes of a row
//            would idle otherwise: the repeat costs no cycle.
//   store    lane 0 of each row puts the 16 words of its record into LDS; the four 64-byte records leave as one 256-byte store, a
//            word per lane.  Rows behind the cut-off leave as zeros, so the table's bytes repeat from pass to pass.
//   loads    the work per window is tiny: what a block costs is the latency of its loads -- the window and result records, then the
//            gathers that depend on them.  collide_kernel is a persistent grid of single-wave workgroups over (trace, block of
//            COL_ROWS = 16 table rows): lane l < 16 fetches the records of row l of the block (one round trip for the block), the
//            rows' values reach the gathering lanes by shuffle.  The records of the workgroup's NEXT block are fetched before the
//            first step of this one, and the gathers of every step -- the first of the next block among them -- are issued before
//            the step in front of it is walked: a workgroup waits for memory once, before its first step.
//   collide_one_kernel   the per-call twin: the same device function over DC-free windows and result records a caller holds.
// The cut-off is the other stages' (stage_windows); the first block of a trace writes nrows[s].  Nothing is shared between
// workgroups, no atomics: nothing depends on the order in which they run.  Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int COL_PACK = 4;               // windows per wave and step, one per 16-lane row
constexpr int COL_STEPS = 4;              // steps per block
constexpr int COL_ROWS = COL_PACK * COL_STEPS;   // table rows per block: lane l < COL_ROWS fetches the records of row l
constexpr int COL_WGS_PER_CU = 8;         // most single-wave workgroups of a launch, per compute unit
constexpr int COL_STRIDE = 17;            // float4 per parked row
constexpr int COL_WORDS = (int)(sizeof(rfid_collision) / sizeof(int));
constexpr int COL_FIRST = 65;             // the first half-bit sample lies index = m + 65 behind the window's start
static_assert(sizeof(rfid_collision) == 64 && COL_PACK * COL_WORDS == 64, "rfid_collision is sixteen words: one word per lane");
static_assert(COL_ROWS <= 64 && (COL_STRIDE * 4) % 64 == 4, "the four rows start four banks apart");
static_assert((N_SYNC - 1) + COL_FIRST + 10 * 15 + 5 < RN16_WIN, "the furthest sample (234) lies inside the window");

RFID_DEVICE float col_dist(float px, float py, float qx, float qy) {
  const float ex = px - qx, ey = py - qy;
  return ex * ex + ey * ey;
}

// 16 bits, the first decided in bit 0 -> MSB first as sent
RFID_DEVICE unsigned col_rev16(unsigned v) {
  v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
  v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
  v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
  return ((v >> 8) & 0xFFu) | ((v & 0xFFu) << 8);
}
// the decoder's sign chain (c bit j: decision j positive): bit j = (c_j != c_j-1), c_-1 positive; as a handle
RFID_DEVICE unsigned col_handle(unsigned c) { return col_rev16((c ^ ((c << 1) | 1u)) & 0xFFFFu); }

// the sync offset of a result's index (tag_decoder_impl.cc:107), held in 0 .. 14 whatever a record says
RFID_DEVICE int col_sync(int index) {
  const int m = index - COL_FIRST;
  return (m < 0) ? 0 : ((m > N_SYNC - 1) ? (N_SYNC - 1) : m);
}

struct ColWin {          // the window of a lane's row (the same in the 16 lanes of a row)
  float dcr, dci, hre, him;
  int bits, stream, seq;
  bool on;               // before the cut-off
};

// One step: the four windows of the wave's rows, p / q the two samples of decision t = lane & 15 of the lane's own row.  -> word
// `lane` of the four records side by side (zeros for a row that is not on).  pts: COL_PACK * COL_STRIDE float4 of LDS, rec: 64 words;
// both may be written again behind the call.
RFID_DEVICE int collide_step(float4 *pts, int *rec, float2 p, float2 q, const ColWin &w, int lane) {
  const int row = lane >> 4, t = lane & 15;
  float4 *mine = pts + row * COL_STRIDE;
  {
    const float dx = (p.x - w.dcr) - (q.x - w.dcr), dy = (p.y - w.dci) - (q.y - w.dci);
    mine[t] = make_float4(dx, dy, dx * dx - dy * dy, (2.0f * dx) * dy);
  }
  wv::wave_sync();
  const float hre = w.hre, him = w.him;
  const float ax = hre * hre - him * him, ay = (2.0f * hre) * him;
  // ---- the start: the square farthest from A, the first of equals ----
  float cx, cy;
  {
    const float4 e = mine[0];
    float far = col_dist(e.z, e.w, ax, ay);
    cx = e.z; cy = e.w;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      const float4 f = mine[j];
      const float g = col_dist(f.z, f.w, ax, ay);
      if (g > far) { far = g; cx = f.z; cy = f.w; }
    }
  }
  // ---- four rounds: the members' mean ----
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    float sx = 0.0f, sy = 0.0f;
    int n = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float4 e = mine[j];
      if (col_dist(e.z, e.w, cx, cy) < col_dist(e.z, e.w, ax, ay)) { sx = sx + e.z; sy = sy + e.w; ++n; }
    }
    if (n) { cx = wv::fdiv(sx, (float)n); cy = wv::fdiv(sy, (float)n); }
  }
  // ---- the last assignment, and the signed sums of the two sets ----
  float ssx = 0.0f, ssy = 0.0f, sdx = 0.0f, sdy = 0.0f, rx = 0.0f, ry = 0.0f;
  int nd = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float4 e = mine[j];
    if (col_dist(e.z, e.w, cx, cy) < col_dist(e.z, e.w, ax, ay)) {
      if (nd == 0) { rx = e.x; ry = e.y; }
      const bool pos = e.x * rx + e.y * ry > 0.0f;
      sdx = sdx + (pos ? e.x : -e.x);
      sdy = sdy + (pos ? e.y : -e.y);
      ++nd;
    } else {
      const bool pos = e.x * hre + e.y * him > 0.0f;
      ssx = ssx + (pos ? e.x : -e.x);
      ssy = ssy + (pos ? e.y : -e.y);
    }
  }
  const int ns = 16 - nd;
  const float hsx = ns ? wv::fdiv(ssx, (float)ns) : hre, hsy = ns ? wv::fdiv(ssy, (float)ns) : him;
  const float hdx = nd ? wv::fdiv(sdx, (float)nd) : 0.0f, hdy = nd ? wv::fdiv(sdy, (float)nd) : 0.0f;
  // ---- every decision the nearest of the four points, the first of equals ----
  unsigned alpha = 0u, beta = 0u;        // bit j: positive
  float resid = 0.0f, sum_sq = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float4 e = mine[j];
    float best = col_dist(e.x, e.y, hsx, hsy);
    int k = 0;
    const float d1 = col_dist(e.x, e.y, -hsx, -hsy), d2 = col_dist(e.x, e.y, hdx, hdy), d3 = col_dist(e.x, e.y, -hdx, -hdy);
    if (d1 < best) { best = d1; k = 1; }
    if (d2 < best) { best = d2; k = 2; }
    if (d3 < best) { best = d3; k = 3; }
    alpha |= ((k == 0 || k == 2) ? 1u : 0u) << j;
    beta |= ((k == 0 || k == 3) ? 1u : 0u) << j;
    resid = resid + best;
    sum_sq = sum_sq + (e.x * e.x + e.y * e.y);
  }
  // ---- handles and labels: A is the stronger tag ----
  unsigned ra = col_handle(alpha), rb = col_handle(beta);
  float h1x = wv::fdiv(hsx + hdx, 2.0f), h1y = wv::fdiv(hsy + hdy, 2.0f);
  float h2x = wv::fdiv(hsx - hdx, 2.0f), h2y = wv::fdiv(hsy - hdy, 2.0f);
  const bool swap = h2x * h2x + h2y * h2y > h1x * h1x + h1y * h1y;
  if (swap) {
    const unsigned u = ra; ra = rb; rb = u;
    float f = h1x; h1x = h2x; h2x = f;
    f = h1y; h1y = h2y; h2y = f;
  }
  const unsigned dec = col_rev16((unsigned)w.bits & 0xFFFFu);
  if (t == 0) {
    int *r = rec + row * COL_WORDS;
    if (w.on) {
      r[0] = w.stream; r[1] = w.seq;
      r[2] = ((dec == ra) ? 1 : 0) | ((dec == rb) ? 2 : 0) | ((nd == 0) ? 4 : 0) | (swap ? 8 : 0);
      r[3] = ns; r[4] = nd; r[5] = (int)ra; r[6] = (int)rb;
      r[7] = (int)wv::f2u(h1x); r[8] = (int)wv::f2u(h1y); r[9] = (int)wv::f2u(h2x); r[10] = (int)wv::f2u(h2y);
      r[11] = (int)wv::f2u(resid); r[12] = (int)wv::f2u(sum_sq); r[13] = (int)wv::f2u(cx); r[14] = (int)wv::f2u(cy);
      r[15] = 0;
    } else {
#pragma unroll
      for (int i = 0; i < COL_WORDS; ++i) r[i] = 0;
    }
  }
  wv::wave_sync();
  const int word = rec[lane];
  wv::wave_sync();   // (the next step overwrites both areas)
  return word;
}

struct ColArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an RN16 window is seq >> 1
  int blocks;                       // ceil(rows / COL_ROWS)
  rfid_collision *table;            // [n_streams][rows]
  int *nrows;                       // [n_streams]: RN16 windows before the cut-off ((n_windows_used + 1) / 2)
};

struct ColBlock {        // a block as the wave holds it
  int strm, r0, nrows;   // its trace, its first row, the trace's rows before the cut-off (the same in every lane)
  int start, m, bits;    // lane l < COL_ROWS: of row r0 + l (zeros behind the cut-off)
  float dcr, dci, hre, him;
};

// the records of block `it`: one window and one result record per lane of the first sixteen, all in flight together
RFID_DEVICE ColBlock col_fetch(const ColArgs &a, int64_t it, int lane) {
  ColBlock b;
  b.strm = (int)(it / a.blocks);
  b.r0 = (int)(it - (int64_t)b.strm * a.blocks) * COL_ROWS;
  b.nrows = (stage_windows(a.p.wcount, a.p.stats, a.p.wmax, b.strm) + 1) >> 1;     // seq = 2 row < nw
  b.start = 0; b.m = 0; b.bits = 0;
  b.dcr = 0.0f; b.dci = 0.0f; b.hre = 0.0f; b.him = 0.0f;
  const int row = b.r0 + lane;
  if (lane < COL_ROWS && row < b.nrows) {
    const int64_t k = (int64_t)b.strm * a.p.wmax + 2 * row;
    const rfid_window *wd = a.p.wtab + k;
    const rfid_decode_result *rs = a.p.res + k;
    b.start = wd->start; b.dcr = wd->dc_re; b.dci = wd->dc_im;
    b.m = col_sync(rs->index); b.hre = rs->h_re; b.him = rs->h_im; b.bits = (int)rs->bits[0];
  }
  return b;
}

struct ColTaps { float2 p, q; };

// the two samples of this lane's decision in step k of block b (zeros behind the cut-off: nothing is read there)
RFID_DEVICE ColTaps col_gather(const ColArgs &a, const ColBlock &b, int k, int lane) {
  const int src = COL_PACK * k + (lane >> 4), t = lane & 15;
  const int start = wv::shfl(b.start, src), m = wv::shfl(b.m, src);
  ColTaps g;
  g.p = make_float2(0.0f, 0.0f); g.q = make_float2(0.0f, 0.0f);
  if (b.r0 + src < b.nrows) {
    const float2 *y = a.p.y + (int64_t)b.strm * a.p.y_stride + start + (m + COL_FIRST + 10 * t);
    g.p = y[0]; g.q = y[5];
  }
  return g;
}

RFID_KERNEL(64) void collide_kernel(ColArgs a) {
  RFID_SHARED float4 pts[COL_PACK * COL_STRIDE];
  RFID_SHARED int rec[COL_PACK * COL_WORDS];
  const int lane = wv::lane_id();
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  int *table_w = reinterpret_cast<int *>(a.table);
  int64_t it = (int64_t)blockIdx.x;
  if (it >= n_items) return;
  ColBlock cur = col_fetch(a, it, lane);
  ColTaps taps = col_gather(a, cur, 0, lane);
  for (;;) {
    // ---- the next block's records: in flight while this block is walked ----
    const int64_t nit = it + (int64_t)gridDim.x;
    const bool more = nit < n_items;
    ColBlock nxt = cur;
    if (more) nxt = col_fetch(a, nit, lane);
    if (cur.r0 == 0 && lane == 0) a.nrows[cur.strm] = cur.nrows;
#pragma unroll
    for (int k = 0; k < COL_STEPS; ++k) {
      // ---- the next step's gathers (behind the block's last step: the next block's first), then this step ----
      ColTaps ahead;
      ahead.p = make_float2(0.0f, 0.0f); ahead.q = make_float2(0.0f, 0.0f);
      if (k + 1 < COL_STEPS) ahead = col_gather(a, cur, k + 1, lane);
      else if (more) ahead = col_gather(a, nxt, 0, lane);
      const int row0 = cur.r0 + COL_PACK * k, src = COL_PACK * k + (lane >> 4);
      int word = 0;
      if (row0 < cur.nrows) {                 // (else the whole step lies behind the cut-off: zeros)
        ColWin w;
        w.dcr = wv::shfl(cur.dcr, src); w.dci = wv::shfl(cur.dci, src);
        w.hre = wv::shfl(cur.hre, src); w.him = wv::shfl(cur.him, src);
        w.bits = wv::shfl(cur.bits, src);
        w.stream = cur.strm; w.seq = 2 * (cur.r0 + src);
        w.on = cur.r0 + src < cur.nrows;
        word = collide_step(pts, rec, taps.p, taps.q, w, lane);
      }
      const int my_row = cur.r0 + src;
      if (my_row < a.rows) table_w[((int64_t)cur.strm * a.rows + my_row) * COL_WORDS + (lane & 15)] = word;
      taps = ahead;
    }
    if (!more) break;
    cur = nxt;
    it = nit;
  }
}

// ---- the per-call twin: n windows of RN16_WIN gated, DC-free samples a caller holds, and their result records -> one record each ----
RFID_KERNEL(64) void collide_one_kernel(const float2 *gated, const rfid_decode_result *res, int n, rfid_collision *out) {
  RFID_SHARED float4 pts[COL_PACK * COL_STRIDE];
  RFID_SHARED int rec[COL_PACK * COL_WORDS];
  const int lane = wv::lane_id(), t = lane & 15;
  const int packs = (n + COL_PACK - 1) / COL_PACK;
  int *out_w = reinterpret_cast<int *>(out);
  for (int it = (int)blockIdx.x; it < packs; it += (int)gridDim.x) {
    const int k = it * COL_PACK + (lane >> 4);
    ColWin w;
    w.dcr = 0.0f; w.dci = 0.0f; w.hre = 0.0f; w.him = 0.0f; w.bits = 0; w.stream = 0; w.seq = k; w.on = k < n;
    float2 p = make_float2(0.0f, 0.0f), q = make_float2(0.0f, 0.0f);
    if (w.on) {
      const rfid_decode_result *rs = res + k;
      w.hre = rs->h_re; w.him = rs->h_im; w.bits = (int)rs->bits[0];
      const float2 *y = gated + (int64_t)k * RN16_WIN + (col_sync(rs->index) + COL_FIRST + 10 * t);
      p = y[0]; q = y[5];
    }
    const int word = collide_step(pts, rec, p, q, w, lane);
    if (w.on) out_w[(int64_t)k * COL_WORDS + t] = word;
  }
}

}  // namespace rfidk
