// rfid_repair.hpp -- the repair stage of the batched path: behind the inventory of a pass, one rfid_repair per EPC window
// before the TERMINATED cut-off.  A window whose CRC-16 failed is searched for the one to three WEAKEST of its 128 sign
// decisions (tag_decoder_impl.cc:171-190) whose reversal makes the frame pass check_crc (:401-445).  The decoder is
// differential -- bit j = "sign j equals sign j - 1" -- so reversing decision j toggles frame bits j and j + 1 (bit 127 only
// for j = 127).  No counterpart in the reference: it is what a caller would otherwise do on the host from every failed
// window's 1 370 gated samples.  A repair is never counted as a read: it is reported on its own, with the entry of the
// same trace's inventory that holds the repaired frame, if one does.
//
// The definition (include/rfid_mi355x.h, rfid_repair) is in binary32, one rounding per operation: a record is a function of
// the input alone.  The shape:
//   repair_search   a wave-level device function.  Lane l holds a_l and a_(l + 64), a_j = |r_j|.
//     candidates    eight rounds of a wave minimum over the bit patterns of the a not yet taken (non-negative: they order as
//                   the values do), then the first lane that holds the minimum by ballot, j < 64 before j >= 64: the eight
//                   smallest (a, j) in order, known to every lane.  Nothing goes through LDS.
//     syndromes     CRC-16 is GF(2)-linear (Crc16Table): the frame passes when the XOR of the columns of its set bits equals a
//                   constant.  A frame bit's column is C[i] for i < 112 and the bit's own place in the received CRC behind
//                   that; decision j's column is column j XOR column j + 1.
//     masks         the 255 masks four per lane (m = 4 lane + k): XOR of the chosen columns against the window's syndrome,
//                   at most three bits, cost ((0 + a) + a) + a in candidate order.  A lane keeps its cheapest, the smaller m
//                   on equal cost; one wave minimum over the costs' bit patterns and the lowest lane that holds it give the
//                   winner -- lanes are in the order of m.
//   repair_kernel   single-wave workgroups over (trace, block of 16 table rows), one row per lane of the first sixteen:
//                   stage_windows for the cut-off, then every lane fetches its own row's window and result record (all
//                   twelve words: stage_fetch blanks the fields of a failed window, which are the ones needed here; the test
//                   for a read is the same) and the trace's first 64 inventory entries sit one per lane; one ballot finds the
//                   failed rows.  They are taken one after the other -- the search is a chain of wave operations -- so the
//                   chain is kept short: a failed row's record reaches all lanes by readlane, not by a second fetch, the
//                   gathers of the next failed row (as quality_kernel's) are in flight during a search, the CRC columns a lane
//                   needs are read once per wave, and the entry lookup compares registers (entries behind the first 64 are
//                   read when a trace has them).  A clean block costs one round trip.  Every row before the cut-off is
//                   written, rows behind it are zeroed; the block's number of repaired rows goes to counts[].
//   repair_offsets_kernel / repair_pack_kernel   the exclusive scan over the blocks' counts (scan_share for the threads' shares,
//                   wave scans and the waves' sums over them) and the copy of the repaired rows, block by block, ranks by
//                   ballot: ordered by (stream, seq), every place computed.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int REP_CAND = RFID_REPAIR_CANDIDATES;
constexpr int REP_MAX_FLIPS = RFID_REPAIR_MAX_FLIPS;
constexpr int REP_ROWS = 16;              // table rows per workgroup and step, one per lane of the first sixteen: a wave takes its
                                          // failed rows one after the other, so short blocks keep that chain short
constexpr int REP_WGS_PER_CU = 8;         // most single-wave workgroups of a launch, per compute unit
constexpr int REP_WORDS = (int)(sizeof(rfid_repair) / sizeof(int));
static_assert(sizeof(rfid_repair) == 48 && REP_WORDS == 12, "rfid_repair is twelve words");
static_assert(REP_CAND == 8 && REP_MAX_FLIPS == 3, "four masks per lane, three flip bytes");

struct RepairFound {     // (the same in every lane)
  int n_flips, flips;
  float cost;
  uint32_t f[4];
};

// the CRC syndrome column of frame bit i: the register's share for a message bit, the bit's place in the received CRC (bit
// 112 is its most significant) behind the message; nothing behind the frame
RFID_DEVICE unsigned rep_column(int i) {
  if (i < 112) return g_crc16.c[i];
  return (i < 128) ? (1u << (127 - i)) : 0u;
}

// what a lane keeps of the table for all the windows it meets: the columns of frame bits and of decisions lane / lane + 64
struct RepairCols {
  unsigned c0, c1;      // frame bit lane, lane + 64
  unsigned d0, d1;      // decision lane, lane + 64: its bit's column XOR the next bit's
  unsigned k;           // what the syndrome of the all-zero frame is
};

RFID_DEVICE RepairCols repair_cols(int lane) {
  RepairCols t;
  t.c0 = rep_column(lane); t.c1 = rep_column(lane + 64);
  t.d0 = t.c0 ^ rep_column(lane + 1); t.d1 = t.c1 ^ rep_column(lane + 65);
  t.k = (unsigned)g_crc16.k ^ 0xFFFFu;
  return t;
}

// a0 / a1: |r_j| of j = lane / lane + 64.  b0 / b1: the window's frame bits 0..63 / 64..127.
RFID_DEVICE RepairFound repair_search(const RepairCols &t, float a0, float a1, uint64_t b0, uint64_t b1, int lane) {
  // ---- the window's syndrome: 0 when the frame passes ----
  unsigned syn = 0;
  if ((b0 >> lane) & 1ull) syn ^= t.c0;
  if ((b1 >> lane) & 1ull) syn ^= t.c1;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) syn ^= wv::shfl_xor(syn, off);
  syn ^= t.k;
  // ---- the eight smallest (a, j) ----
  constexpr unsigned TAKEN = 0xFFFFFFFFu;
  unsigned k0 = wv::f2u(a0), k1 = wv::f2u(a1);
  int cj[REP_CAND];
  float ca[REP_CAND];
  unsigned col[REP_CAND];
#pragma unroll
  for (int i = 0; i < REP_CAND; ++i) {
    unsigned mn = (k1 < k0) ? k1 : k0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned o = wv::shfl_xor(mn, off);
      mn = (o < mn) ? o : mn;
    }
    const uint64_t lo = wv::ballot(k0 == mn), hi = wv::ballot(k1 == mn);
    const int j = lo ? wv::ffs64(lo) : (64 + (wv::ffs64(hi) & 63));
    if (lane == (j & 63)) {
      if (j < 64) k0 = TAKEN; else k1 = TAKEN;
    }
    cj[i] = j; ca[i] = wv::u2f(mn);
    col[i] = (unsigned)wv::readlane((int)((j < 64) ? t.d0 : t.d1), j & 63);
  }
  // ---- the masks, four per lane ----
  unsigned best = TAKEN;      // bit pattern of the cheapest passing mask's cost
  int best_m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int m = 4 * lane + k;
    unsigned x = 0;
    float cost = 0.0f;
    int n = 0;
#pragma unroll
    for (int i = 0; i < REP_CAND; ++i)
      if ((m >> i) & 1) { x ^= col[i]; cost = cost + ca[i]; ++n; }
    const unsigned key = wv::f2u(cost);
    if (n >= 1 && n <= REP_MAX_FLIPS && x == syn && (best_m == 0 || key < best)) { best = key; best_m = m; }
  }
  unsigned mn = (best_m != 0) ? best : TAKEN;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned o = wv::shfl_xor(mn, off);
    mn = (o < mn) ? o : mn;
  }
  const uint64_t won = wv::ballot(best_m != 0 && best == mn);
  RepairFound r;
  r.n_flips = 0; r.flips = -1; r.cost = 0.0f;
  r.f[0] = r.f[1] = r.f[2] = r.f[3] = 0u;
  if (!won) return r;
  const int lead = wv::ffs64(won);
  const int m = wv::readlane(best_m, lead);
  // ---- the winner: its decisions in ascending j, the frame with their bits toggled ----
  int x0 = 255, x1 = 255, x2 = 255, n = 0;
  uint64_t f0 = b0, f1 = b1;
#pragma unroll
  for (int i = 0; i < REP_CAND; ++i) {
    if (!((m >> i) & 1)) continue;
    const int j = cj[i];
    ++n;
    if (j < x0) { x2 = x1; x1 = x0; x0 = j; }
    else if (j < x1) { x2 = x1; x1 = j; }
    else if (j < x2) { x2 = j; }
    if (j < 64) f0 ^= 1ull << j; else f1 ^= 1ull << (j - 64);
    if (j + 1 < 64) f0 ^= 1ull << (j + 1); else if (j + 1 < 128) f1 ^= 1ull << (j + 1 - 64);
  }
  r.n_flips = n;
  r.flips = x0 | (x1 << 8) | (x2 << 16) | (int)0xFF000000u;
  r.cost = wv::u2f(mn);
  r.f[0] = (uint32_t)f0; r.f[1] = (uint32_t)(f0 >> 32); r.f[2] = (uint32_t)f1; r.f[3] = (uint32_t)(f1 >> 32);
  return r;
}

// |r_j| of j = lane and lane + 64 of one window: the decoder's own gather (epc_gather) and the decision value as quality_kernel
// forms it
RFID_DEVICE void repair_gather(const float2 *src, float dcr, float dci, float h_re, float h_im, float T, float fidx, int lane,
                               float &a0, float &a1) {
  const float nhim = -h_im;
  float2 pa, qa, pb, qb;
  epc_gather(src, T, fidx, lane, pa, qa, pb, qb);
  const float dx0 = (pa.x - dcr) - (qa.x - dcr), dy0 = (pa.y - dci) - (qa.y - dci);
  const float dx1 = (pb.x - dcr) - (qb.x - dcr), dy1 = (pb.y - dci) - (qb.y - dci);
  a0 = __builtin_fabsf(dx0 * h_re - dy0 * nhim);
  a1 = __builtin_fabsf(dx1 * h_re - dy1 * nhim);
}

// one window as the search needs it: where its samples lie and what its result says (12 words of it)
struct RepairWin {
  int start, dcr, dci;                 // rfid_window (bit patterns)
  int type, index, h_re, h_im, T;      // rfid_decode_result (bit patterns)
  int b[4];
  int crc_ok;
};

RFID_DEVICE RepairWin repair_fetch(const rfid_window *wd, const rfid_decode_result *rs) {
  static_assert(sizeof(rfid_decode_result) == 48, "rfid_decode_result is read as 12 words");
  RepairWin w;
  w.start = wd->start; w.dcr = (int)wv::f2u(wd->dc_re); w.dci = (int)wv::f2u(wd->dc_im);
  const int *p = reinterpret_cast<const int *>(rs);
  int n_bits, tag_id;
  wv::load4_i32(p, w.type, w.index, w.h_re, w.h_im);
  wv::load4_i32(p + 4, w.T, w.b[0], w.b[1], w.b[2]);
  wv::load4_i32(p + 8, w.b[3], n_bits, w.crc_ok, tag_id);
  return w;
}

// lane `src`'s window in every lane
RFID_DEVICE RepairWin repair_bcast(const RepairWin &w, int src) {
  RepairWin u;
  u.start = wv::readlane(w.start, src); u.dcr = wv::readlane(w.dcr, src); u.dci = wv::readlane(w.dci, src);
  u.type = wv::readlane(w.type, src); u.index = wv::readlane(w.index, src);
  u.h_re = wv::readlane(w.h_re, src); u.h_im = wv::readlane(w.h_im, src); u.T = wv::readlane(w.T, src);
#pragma unroll
  for (int i = 0; i < 4; ++i) u.b[i] = wv::readlane(w.b[i], src);
  u.crc_ok = wv::readlane(w.crc_ok, src);
  return u;
}

// the gathers of a window (the same in every lane) from the trace's (or the caller's) samples
RFID_DEVICE void repair_gather_win(const float2 *y, const RepairWin &u, int lane, float &a0, float &a1) {
  repair_gather(y + u.start, wv::u2f((uint32_t)u.dcr), wv::u2f((uint32_t)u.dci), wv::u2f((uint32_t)u.h_re), wv::u2f((uint32_t)u.h_im),
                wv::u2f((uint32_t)u.T), (float)u.index, lane, a0, a1);
}

RFID_DEVICE RepairFound repair_search_win(const RepairCols &t, const RepairWin &u, float a0, float a1, int lane) {
  const uint64_t b0 = (uint64_t)(uint32_t)u.b[0] | ((uint64_t)(uint32_t)u.b[1] << 32);
  const uint64_t b1 = (uint64_t)(uint32_t)u.b[2] | ((uint64_t)(uint32_t)u.b[3] << 32);
  return repair_search(t, a0, a1, b0, b1, lane);
}

struct RepArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / REP_ROWS)
  const rfid_tag_entry *ent;        // [n_streams][max_tags]: the inventory of the same pass
  const int *ent_counts;            // [n_streams]: its entries per trace (0 when the trace overflowed)
  const int *ent_over;              // [n_streams]: 1 = the trace overflowed the inventory
  int max_tags;
  rfid_repair *table;               // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
  int *counts;                      // [n_streams][blocks]: repaired rows of the block
};

RFID_KERNEL(64) void repair_kernel(RepArgs a) {
  const int lane = wv::lane_id();
  const RepairCols cols = repair_cols(lane);
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int s = (int)(it / a.blocks);
    const int r0 = (int)(it - (int64_t)s * a.blocks) * REP_ROWS;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, s);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[s] = nrows;
    const int my_row = r0 + lane;
    const bool mine = lane < REP_ROWS && my_row < a.rows;      // (this lane stores a row)
    const bool on = lane < REP_ROWS && my_row < nrows;
    const int k = 2 * my_row + 1;
    rfid_repair rec;
    rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.n_flips = 0; rec.flips = 0; rec.cost = 0.0f; rec.entry = 0;
    rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
    int repaired = 0;
    if (r0 < nrows) {
      // ---- every lane its own row: window and result, all rows of the block in flight together ----
      RepairWin w;
      w.start = w.dcr = w.dci = w.type = w.index = w.h_re = w.h_im = w.T = w.crc_ok = 0;
      w.b[0] = w.b[1] = w.b[2] = w.b[3] = 0;
      if (on) w = repair_fetch(a.p.wtab + ((int64_t)s * a.p.wmax + k), a.p.res + ((int64_t)s * a.p.wmax + k));
      const bool ok = w.type == RFID_DECODE_EPC && w.crc_ok == 1;      // (a read, as stage_fetch has it)
      const int over = a.ent_over[s] ? 2 : 0;
      const int E = over ? 0 : a.ent_counts[s];
      // the trace's first 64 inventory entries, one per lane (the rule: a handful of tags); those behind them are read when needed
      const rfid_tag_entry *ent = a.ent + (int64_t)s * a.max_tags;
      uint32_t ef[4] = {0u, 0u, 0u, 0u};
      if (lane < E) { ef[0] = ent[lane].frame[0]; ef[1] = ent[lane].frame[1]; ef[2] = ent[lane].frame[2]; ef[3] = ent[lane].frame[3]; }
      if (on) {
        rec.stream = s; rec.seq = k; rec.start = w.start;
        rec.flags = (ok ? 1 : 0) | over;
        rec.flips = -1; rec.entry = -1;
      }
      // ---- the failed rows of the block, one after the other; the gathers of the next one are in flight during a search ----
      const float2 *y = a.p.y + (int64_t)s * a.p.y_stride;
      uint64_t todo = wv::ballot(on && !ok);
      RepairWin u = w;
      float a0 = 0.0f, a1 = 0.0f;
      if (todo) {
        u = repair_bcast(w, wv::ffs64(todo));
        repair_gather_win(y, u, lane, a0, a1);
      }
      while (todo) {
        const int lead = wv::ffs64(todo);
        todo &= todo - 1ull;
        const RepairWin cur = u;
        const float c0 = a0, c1 = a1;
        if (todo) {
          u = repair_bcast(w, wv::ffs64(todo));
          repair_gather_win(y, u, lane, a0, a1);
        }
        const RepairFound f = repair_search_win(cols, cur, c0, c1, lane);
        if (f.n_flips == 0) continue;
        // the entry of this trace's inventory that holds the repaired frame: the lowest index among the lanes that match
        int entry = -1;
        {
          const uint64_t m = wv::ballot(lane < E && ef[0] == f.f[0] && ef[1] == f.f[1] && ef[2] == f.f[2] && ef[3] == f.f[3]);
          if (m) entry = wv::ffs64(m);
        }
        for (int base = 64; entry < 0 && base < E; base += 64) {
          const int e = base + lane;
          bool hit = false;
          if (e < E) {
            const uint32_t *g = ent[e].frame;
            hit = g[0] == f.f[0] && g[1] == f.f[1] && g[2] == f.f[2] && g[3] == f.f[3];
          }
          const uint64_t m = wv::ballot(hit);
          if (m) entry = base + wv::ffs64(m);
        }
        ++repaired;
        if (lane == lead) {
          rec.n_flips = f.n_flips; rec.flips = f.flips; rec.cost = f.cost; rec.entry = entry;
          rec.frame[0] = f.f[0]; rec.frame[1] = f.f[1]; rec.frame[2] = f.f[2]; rec.frame[3] = f.f[3];
        }
      }
    }
    if (mine) a.table[(int64_t)s * a.rows + my_row] = rec;     // (behind the cut-off: zeros)
    if (lane == 0) a.counts[it] = repaired;
  }
}

// ---- the repaired rows of all traces in one piece, ordered by (stream, seq): offsets (one workgroup), then the copy -----------
struct RepPackArgs {
  const rfid_repair *table;         // [n_streams][rows]
  const int *counts;                // [n_streams][blocks]
  int n_streams, rows, blocks;
  int *offsets;                     // [n_streams][blocks]: repaired rows of the blocks before this one
  int *head;                        // [0] repaired rows in all
  rfid_repair *packed;              // [cap]
  int64_t cap;
};

// (the share of a thread as in inventory_offsets_kernel; the scan over the threads by wave scans and the waves' sums, not by one
// thread's walk over all partial sums: with a thousand traces that walk alone would take as long as the search)
RFID_KERNEL(INV_SCAN_THREADS) void repair_offsets_kernel(RepPackArgs a) {
  RFID_SHARED int wsum[INV_SCAN_THREADS / 64];
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
  const ScanShare sh = scan_share(a.n_streams * a.blocks, tid, nthr);     // (< 2^31: the table's rows are)
  int sum = 0;
  for (int b = sh.b0; b < sh.b1; ++b) sum += a.counts[b];
  const int incl = wv::scan_add(sum);
  if (lane == 63) wsum[wave] = incl;
  wv::block_sync();
  int run = incl - sum, total = 0;
  for (int w = 0; w < (nthr >> 6); ++w) {
    const int v = wsum[w];
    if (w < wave) run += v;
    total += v;
  }
  if (tid == 0) a.head[0] = total;
  for (int b = sh.b0; b < sh.b1; ++b) { a.offsets[b] = run; run += a.counts[b]; }
}

RFID_KERNEL(64) void repair_pack_kernel(RepPackArgs a) {
  const int lane = wv::lane_id();
  const int64_t n_items = (int64_t)a.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    if (a.counts[it] == 0) continue;
    const int s = (int)(it / a.blocks);
    const int row = (int)(it - (int64_t)s * a.blocks) * REP_ROWS + lane;
    const int *src = reinterpret_cast<const int *>(a.table + ((int64_t)s * a.rows + (row < a.rows ? row : 0)));
    const bool keep = lane < REP_ROWS && row < a.rows && src[4] > 0;      // n_flips
    const uint64_t m = wv::ballot(keep);
    const int64_t pos = (int64_t)a.offsets[it] + wv::popc64(m & ((1ull << lane) - 1ull));
    if (keep && pos < a.cap) {
      int *dst = reinterpret_cast<int *>(a.packed + pos);
#pragma unroll
      for (int w = 0; w < REP_WORDS; w += 4) {
        int v0, v1, v2, v3;
        wv::load4_i32(src + w, v0, v1, v2, v3);
        dst[w] = v0; dst[w + 1] = v1; dst[w + 2] = v2; dst[w + 3] = v3;
      }
    }
  }
}

// ---- one caller-supplied window (rfid_repair_window): the same gather and search, one wave ---------------------------------------
RFID_KERNEL(64) void repair_one_kernel(const float2 *gated, const rfid_decode_result *res, rfid_repair *out) {
  const int lane = wv::lane_id();
  const RepairCols cols = repair_cols(lane);
  rfid_window wd;
  wd.stream = 0; wd.seq = 0; wd.start = 0; wd.type = RFID_DECODE_EPC; wd.dc_re = 0.0f; wd.dc_im = 0.0f;      // (DC-free already)
  const RepairWin u = repair_fetch(&wd, res);
  rfid_repair rec;
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = u.crc_ok & 1; rec.n_flips = 0; rec.flips = -1; rec.cost = 0.0f;
  rec.entry = -1;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
  if (!rec.flags) {
    float a0, a1;
    repair_gather_win(gated, u, lane, a0, a1);
    const RepairFound f = repair_search_win(cols, u, a0, a1, lane);
    if (f.n_flips > 0) {
      rec.n_flips = f.n_flips; rec.flips = f.flips; rec.cost = f.cost;
      rec.frame[0] = f.f[0]; rec.frame[1] = f.f[1]; rec.frame[2] = f.f[2]; rec.frame[3] = f.f[3];
    }
  }
  if (lane == 0) *out = rec;
}

}  // namespace rfidk
