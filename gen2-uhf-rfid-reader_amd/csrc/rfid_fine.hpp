// rfid_fine.hpp -- the fine-channel stage of the batched path: behind the tracks of a pass, one rfid_read_fine per EPC window
// before the TERMINATED cut-off, CRC-verified or not -- the data-aided channel estimate of the read.  The decoder's h_est is the
// mean of six matched-filter samples of the preamble relative to the gate's dc_est; the 128 bits behind it carry 256 more half-bit
// samples of the same channel, and once the frame bits are known so are their polarities: with g_j the decoder's sign chain
// (fm0_decide, tag_decoder_impl.cc:171-190: the sign changes with every 1 bit), sum_j g_j (s_a - s_b) is 128 times the channel,
// free of dc_est, with a noise some 3.3 times below h_est's -- and the same sum over 16 bits at a time gives the channel at eight
// points inside the read.  No counterpart in the reference: what a caller would otherwise work out on the host from every gated
// window of a pass (10 960 bytes each).
//
// The definition (include/rfid_mi355x.h, rfid_read_fine) is in binary32, one rounding per operation, every sum in order from
// 0.0f: a record is a function of the input alone.  The kernel's shape is the quality stage's (csrc/rfid_quality.hpp):
//   gather  a wave takes FINE_PACK = 8 EPC windows of one trace at a time (a persistent grid over (trace, pack of rows)); the
//           decoder's gather (epc_gather), two j per lane -- j = lane and lane + 64 -- the gathers of all eight windows in flight together.
//   signs   the four words of frame bits are the same in every lane; the parity of bits 0..j is a masked population count.
//   park    g dx, g dy and dx^2 + dy^2 go to LDS by (window, segment, component), 17 words apart: the 64 walkers -- one per
//           (window, segment) -- start 51 words apart, in 64 different banks, and walk 16 terms of three rows each.
//   totals  24 lanes -- one per (window, total) -- add the eight segment values in order: 16 + 8 dependent additions, not 128.
//   store   the eight 128-byte records are put together in LDS and leave as four 256-byte stores, one word per lane.
// The cut-off is the inventory's and the tracks' (stage_windows).  Rows behind a trace's cut-off are zeroed, so the table's bytes
// repeat from pass to pass.  Single-wave workgroups, nothing shared between them, no atomics: nothing depends on the order in
// which they run.
// table_gather_kernel<FINE_WORDS> (rfid_stage.hpp) then copies the records of the CRC-verified reads into one array aligned with
// the tracks; fine_one_kernel runs the same device functions on one window a caller holds.
// Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int FINE_PACK = 8;              // EPC windows per wave and step
constexpr int FINE_WGS_PER_CU = 8;        // most single-wave workgroups of a launch, per compute unit
constexpr int FINE_SEGS = 8;              // segments of a window
constexpr int FINE_SEG_BITS = 16;         // decisions per segment
constexpr int FINE_ROW = 17;              // words per (window, segment, component): odd, so 3 x 17 = 51 is odd too
constexpr int FINE_WORDS = (int)(sizeof(rfid_read_fine) / sizeof(int));
constexpr int FINE_STORES = FINE_PACK * FINE_WORDS / 64;    // 256-byte stores per pack
static_assert(sizeof(rfid_read_fine) == 128 && FINE_WORDS == 32, "two records per 256-byte store");
static_assert(FINE_PACK * FINE_SEGS == 64, "one walker per lane");
static_assert(FINE_SEGS * FINE_SEG_BITS == 128 && ((3 * FINE_ROW) & 1) == 1, "walkers 51 words apart: one bank each");
// words of a record
constexpr int FINE_W_STREAM = 0, FINE_W_SEQ = 1, FINE_W_START = 2, FINE_W_FLAGS = 3, FINE_W_SUM = 4, FINE_W_RESERVED = 7, FINE_W_SEG = 8;

struct FineArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): EPC windows have odd seq, the row of one is seq >> 1
  rfid_read_fine *table;            // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

struct FineWin {     // what a window's gathers and signs need (the same in every lane)
  const float2 *src;
  float dcr, dci, T, fidx;
  uint64_t b01, b23;                // frame bits 0..63, 64..127
  int start, crc_ok;
};

// a window's result as the stage reads it: index, T, the frame bits, crc_ok (h_est is not used)
RFID_DEVICE void fine_fetch(const rfid_decode_result *rs, FineWin &w) {
  static_assert(sizeof(rfid_decode_result) == 48, "rfid_decode_result is read as 12 words");
  const int *p = reinterpret_cast<const int *>(rs);
  int type, index, h_re, h_im, T, b0, b1, b2, b3, n_bits, crc_ok, tag_id;
  wv::load4_i32(p, type, index, h_re, h_im);
  wv::load4_i32(p + 4, T, b0, b1, b2);
  wv::load4_i32(p + 8, b3, n_bits, crc_ok, tag_id);
  w.T = wv::u2f((uint32_t)T); w.fidx = (float)index;
  w.b01 = (uint64_t)(uint32_t)b0 | ((uint64_t)(uint32_t)b1 << 32);
  w.b23 = (uint64_t)(uint32_t)b2 | ((uint64_t)(uint32_t)b3 << 32);
  w.crc_ok = crc_ok;
}

// where term i of (window u, segment k, component c) lies
RFID_DEVICE int fine_term_at(int u, int k, int c) { return ((u * FINE_SEGS + k) * 3 + c) * FINE_ROW; }

// the six terms of a lane's two decisions, parked by (window, segment, component)
RFID_DEVICE void fine_park(float *term, int u, const FineWin &w, float2 pa, float2 qa, float2 pb, float2 qb, int lane) {
  const float dcr = w.dcr, dci = w.dci;
  // gate output in[i] - dc_est per component, then the difference of the two half-bit samples
  const float dx0 = (pa.x - dcr) - (qa.x - dcr), dy0 = (pa.y - dci) - (qa.y - dci);
  const float dx1 = (pb.x - dcr) - (qb.x - dcr), dy1 = (pb.y - dci) - (qb.y - dci);
  // the sign chain: +1 while the number of set bits among frame bits 0..j is even
  const uint64_t upto = (2ull << lane) - 1ull;               // bits 0..lane (lane 63: all of them)
  const int n0 = wv::popc64(w.b01 & upto), n1 = wv::popc64(w.b01) + wv::popc64(w.b23 & upto);
  const float g0 = (n0 & 1) ? -1.0f : 1.0f, g1 = (n1 & 1) ? -1.0f : 1.0f;
  const int i = lane & (FINE_SEG_BITS - 1), k0 = lane >> 4, k1 = k0 + 4;
  float *t0 = term + fine_term_at(u, k0, 0) + i, *t1 = term + fine_term_at(u, k1, 0) + i;
  t0[0] = g0 * dx0; t0[FINE_ROW] = g0 * dy0; t0[2 * FINE_ROW] = dx0 * dx0 + dy0 * dy0;
  t1[0] = g1 * dx1; t1[FINE_ROW] = g1 * dy1; t1[2 * FINE_ROW] = dx1 * dx1 + dy1 * dy1;
}

// the in-order sums of n_win parked windows into their records (rec: FINE_WORDS words per window): lane 8 u + k walks the three
// rows of segment k of window u, then lane 3 u + c adds the eight segment values of total c
RFID_DEVICE void fine_sums(const float *term, int *rec, int n_win, int lane) {
  if (lane < n_win * FINE_SEGS) {
    const float *t = term + lane * (3 * FINE_ROW);
    float re = 0.0f, im = 0.0f, pw = 0.0f;
#pragma unroll
    for (int i = 0; i < FINE_SEG_BITS; ++i) {
      re = re + t[i]; im = im + t[FINE_ROW + i]; pw = pw + t[2 * FINE_ROW + i];
    }
    int *r = rec + (lane >> 3) * FINE_WORDS + FINE_W_SEG + (lane & 7);
    r[0] = (int)wv::f2u(re); r[FINE_SEGS] = (int)wv::f2u(im); r[2 * FINE_SEGS] = (int)wv::f2u(pw);
  }
  wv::wave_sync();
  if (lane < n_win * 3) {
    const int u = lane / 3, c = lane - 3 * u;
    const int *sv = rec + u * FINE_WORDS + FINE_W_SEG + c * FINE_SEGS;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < FINE_SEGS; ++k) acc = acc + wv::u2f((uint32_t)sv[k]);
    rec[u * FINE_WORDS + FINE_W_SUM + c] = (int)wv::f2u(acc);
  }
  wv::wave_sync();
}

RFID_KERNEL(64) void fine_kernel(FineArgs a) {
  RFID_SHARED float term[FINE_PACK * FINE_SEGS * 3 * FINE_ROW];
  RFID_SHARED int rec[FINE_PACK * FINE_WORDS];
  const int lane = wv::lane_id();
  const int packs_per = (a.rows + FINE_PACK - 1) / FINE_PACK;
  const int64_t n_items = (int64_t)a.p.n_streams * packs_per;
  int *table_w = reinterpret_cast<int *>(a.table);
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int s = (int)(it / packs_per);
    const int r0 = (int)(it - (int64_t)s * packs_per) * FINE_PACK;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, s);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[s] = nrows;
    int *out = table_w + ((int64_t)s * a.rows + r0) * FINE_WORDS + lane;     // (store q: 64 q words further on, rows r0 + 2 q, + 1)
    if (r0 >= nrows) {                     // behind the cut-off
#pragma unroll
      for (int q = 0; q < FINE_STORES; ++q)
        if (r0 + 2 * q + (lane >> 5) < a.rows) out[64 * q] = 0;
      continue;
    }
    // ---- the eight windows: record, result, the 4 x 8 gathers ----
    FineWin w[FINE_PACK];
    float2 pa[FINE_PACK], qa[FINE_PACK], pb[FINE_PACK], qb[FINE_PACK];
#pragma unroll
    for (int u = 0; u < FINE_PACK; ++u) {
      const int row = (r0 + u < nrows) ? (r0 + u) : r0;      // (a row behind the cut-off: the pack's first, its terms unused)
      const int64_t k = (int64_t)s * a.p.wmax + (2 * row + 1);
      const rfid_window wd = a.p.wtab[k];
      fine_fetch(a.p.res + k, w[u]);
      w[u].src = a.p.y + (int64_t)s * a.p.y_stride + wd.start;
      w[u].dcr = wd.dc_re; w[u].dci = wd.dc_im;
      w[u].start = wd.start;
    }
#pragma unroll
    for (int u = 0; u < FINE_PACK; ++u) epc_gather(w[u].src, w[u].T, w[u].fidx, lane, pa[u], qa[u], pb[u], qb[u]);
#pragma unroll
    for (int u = 0; u < FINE_PACK; ++u) {
      fine_park(term, u, w[u], pa[u], qa[u], pb[u], qb[u], lane);
      if (lane == 0) {
        int *r = rec + u * FINE_WORDS;
        r[FINE_W_STREAM] = s; r[FINE_W_SEQ] = 2 * (r0 + u) + 1; r[FINE_W_START] = w[u].start; r[FINE_W_FLAGS] = w[u].crc_ok & 1;
        r[FINE_W_RESERVED] = 0;
      }
    }
    wv::wave_sync();
    fine_sums(term, rec, FINE_PACK, lane);
    // ---- two records per store; the rows of this pack behind the cut-off are zero ----
#pragma unroll
    for (int q = 0; q < FINE_STORES; ++q) {
      const int row = r0 + 2 * q + (lane >> 5);
      if (row < a.rows) out[64 * q] = (row < nrows) ? rec[64 * q + lane] : 0;
    }
    wv::wave_sync();   // (the next pack overwrites both areas)
  }
}

// ---- one caller-supplied window (rfid_fine_window): the same gather, signs and sums, one wave -----------------------------------
RFID_KERNEL(64) void fine_one_kernel(const float2 *gated, const rfid_decode_result *res, rfid_read_fine *out) {
  RFID_SHARED float term[FINE_SEGS * 3 * FINE_ROW];
  RFID_SHARED int rec[FINE_WORDS];
  const int lane = wv::lane_id();
  FineWin w;
  fine_fetch(res, w);
  w.src = gated; w.dcr = 0.0f; w.dci = 0.0f; w.start = 0;      // (DC-free already)
  float2 pa, qa, pb, qb;
  epc_gather(w.src, w.T, w.fidx, lane, pa, qa, pb, qb);
  fine_park(term, 0, w, pa, qa, pb, qb, lane);
  if (lane < FINE_W_SEG) rec[lane] = (lane == FINE_W_FLAGS) ? (w.crc_ok & 1) : 0;
  wv::wave_sync();
  fine_sums(term, rec, 1, lane);
  if (lane < FINE_WORDS) reinterpret_cast<int *>(out)[lane] = rec[lane];
}

}  // namespace rfidk
