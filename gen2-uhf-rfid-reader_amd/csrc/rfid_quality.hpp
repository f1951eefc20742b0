// rfid_quality.hpp -- the read-quality stage of the batched path: behind the tracks of a pass, one rfid_read_quality per EPC
// window before the TERMINATED cut-off, CRC-verified or not -- how far the 128 decision values of tag_detection_EPC
// (tag_decoder_impl.cc:171-190) stand above what lies in quadrature to them.  The tag modulates along h_est, so
// r_j = Re((s_a - s_b) conj(h_est)) carries the signal and q_j = Im(...) noise and interference only: sum r^2 / sum q^2 tells
// a weak tag from an empty or collided slot, min |r| says which bit was nearest to flipping.  No counterpart in the reference:
// it is what a caller would otherwise work out on the host from every gated window of a pass (10 960 bytes each).
//
// The definition (include/rfid_mi355x.h, rfid_read_quality) is in binary32, one rounding per operation, the three sums in the
// order of j: a record is a function of the input alone.  The kernel's shape:
//   gather  a wave takes QUAL_PACK = 8 EPC windows of one trace at a time (a persistent grid over (trace, pack of rows)).  Only
//           512 of a window's 1 370 samples are touched, 40 bytes apart: they are gathered straight from global memory, as the
//           RN16 decoder does (the decoder streamed them through L2 a moment ago), two j per lane -- j = lane and lane + 64 --
//           and the gathers of all eight windows are in flight together.  |r|, r^2 and q^2 are formed in registers.
//   minimum a wave minimum of min(|r_lane|, |r_lane+64|), then the first lane that holds it by ballot: among j < 64 first,
//           among j >= 64 only when none of those does.
//   sums    the 3 x 128 terms of a window are parked in LDS (rows 129 floats apart: the walkers' rows start in different
//           banks) and 24 lanes -- one per (window, sum) -- walk a row each, from 0.0f in the order of j: 128 dependent
//           additions for eight windows, against the 20 x 256 of the decoder's half-period search for three.
//   store   the eight 32-byte records are put together in LDS and leave as one 256-byte row of the table, one word per lane.
// The cut-off is the inventory's and the tracks' (stage_windows).  Rows behind a trace's cut-off are zeroed, so the table's
// bytes repeat from pass to pass.  Single-wave workgroups, nothing shared between them, no atomics: nothing depends on the
// order in which they run.
// table_gather_kernel<QUAL_WORDS> (rfid_stage.hpp) then copies the records of the CRC-verified reads into one array aligned
// with the tracks.
// Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int QUAL_PACK = 8;              // EPC windows per wave and step
constexpr int QUAL_WGS_PER_CU = 8;        // most single-wave workgroups of a launch, per compute unit
constexpr int QUAL_TERM_STRIDE = 129;     // = 1 mod 32
constexpr int QUAL_WORDS = (int)(sizeof(rfid_read_quality) / sizeof(int));
static_assert(sizeof(rfid_read_quality) == 32 && QUAL_PACK * QUAL_WORDS == 64, "one word per lane");
static_assert(QUAL_PACK * 3 <= 32, "one bank per walker");

struct QualArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): EPC windows have odd seq, the row of one is seq >> 1
  rfid_read_quality *table;         // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

// The decision value r and its quadrature counterpart q of one decision from its two half-bit samples p and s (the definition's
// expressions: the gate's output in[i] - dc_est per component, then the difference of the two).  One copy: the match stage
// (rfid_match.hpp) correlates the same r_j.
RFID_DEVICE void quality_rq(float2 p, float2 s, float dcr, float dci, float h_re, float h_im, float &r, float &q) {
  const float nhim = -h_im;
  const float dx = (p.x - dcr) - (s.x - dcr), dy = (p.y - dci) - (s.y - dci);
  r = dx * h_re - dy * nhim;
  q = dy * h_re - dx * h_im;
}

// (((0.0f + t_0) + t_1) + ...) + t_127 over 128 terms in LDS, ABS: over their magnitudes -- the in-order sums of the definition
template <bool ABS>
RFID_DEVICE float quality_sum128(const float *t) {
  float acc = 0.0f;
#pragma unroll 16
  for (int j = 0; j < 128; ++j) acc = acc + (ABS ? __builtin_fabsf(t[j]) : t[j]);
  return acc;
}

struct QualWin {     // what a window's gathers need (the same in every lane)
  const float2 *src;
  float dcr, dci, h_re, h_im, T, fidx;
  int crc_ok;
};

RFID_KERNEL(64) void quality_kernel(QualArgs a) {
  RFID_SHARED float term[QUAL_PACK * 3 * QUAL_TERM_STRIDE];
  RFID_SHARED int rec[QUAL_PACK * QUAL_WORDS];
  const int lane = wv::lane_id();
  const int packs_per = (a.rows + QUAL_PACK - 1) / QUAL_PACK;
  const int64_t n_items = (int64_t)a.p.n_streams * packs_per;
  int *table_w = reinterpret_cast<int *>(a.table);
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int s = (int)(it / packs_per);
    const int r0 = (int)(it - (int64_t)s * packs_per) * QUAL_PACK;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, s);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[s] = nrows;
    const int my_row = r0 + (lane >> 3);   // (the record this lane stores a word of)
    int *out = table_w + ((int64_t)s * a.rows + my_row) * QUAL_WORDS + (lane & 7);
    if (r0 >= nrows) {                     // behind the cut-off
      if (my_row < a.rows) *out = 0;
      continue;
    }
    // ---- the eight windows: record, result, the 4 x 8 gathers ----
    QualWin w[QUAL_PACK];
    float2 pa[QUAL_PACK], qa[QUAL_PACK], pb[QUAL_PACK], qb[QUAL_PACK];
#pragma unroll
    for (int u = 0; u < QUAL_PACK; ++u) {
      const int row = (r0 + u < nrows) ? (r0 + u) : r0;      // (a row behind the cut-off: the pack's first, its terms unused)
      const int64_t k = (int64_t)s * a.p.wmax + (2 * row + 1);
      const rfid_window wd = a.p.wtab[k];
      const int *p = reinterpret_cast<const int *>(a.p.res + k);
      int t0, t1, t2, t3, t4, d0, d1, d2;
      wv::load4_i32(p, t0, t1, t2, t3);                      // type, index, h_re, h_im
      wv::load4_i32(p + 4, t4, d0, d1, d2);                  // T, bits[0..2]
      w[u].crc_ok = p[10];
      w[u].src = a.p.y + (int64_t)s * a.p.y_stride + wd.start;
      w[u].dcr = wd.dc_re; w[u].dci = wd.dc_im;
      w[u].h_re = wv::u2f((uint32_t)t2); w[u].h_im = wv::u2f((uint32_t)t3); w[u].T = wv::u2f((uint32_t)t4);
      w[u].fidx = (float)t1;
    }
#pragma unroll
    for (int u = 0; u < QUAL_PACK; ++u) epc_gather(w[u].src, w[u].T, w[u].fidx, lane, pa[u], qa[u], pb[u], qb[u]);
    // ---- terms, minimum ----
#pragma unroll
    for (int u = 0; u < QUAL_PACK; ++u) {
      float r0v, q0v, r1v, q1v;
      quality_rq(pa[u], qa[u], w[u].dcr, w[u].dci, w[u].h_re, w[u].h_im, r0v, q0v);
      quality_rq(pb[u], qb[u], w[u].dcr, w[u].dci, w[u].h_re, w[u].h_im, r1v, q1v);
      const float a0 = __builtin_fabsf(r0v), a1 = __builtin_fabsf(r1v);
      float *t = term + (u * 3) * QUAL_TERM_STRIDE;
      t[lane] = a0; t[lane + 64] = a1;
      t[QUAL_TERM_STRIDE + lane] = r0v * r0v; t[QUAL_TERM_STRIDE + lane + 64] = r1v * r1v;
      t[2 * QUAL_TERM_STRIDE + lane] = q0v * q0v; t[2 * QUAL_TERM_STRIDE + lane + 64] = q1v * q1v;
      float mn = (a1 < a0) ? a1 : a0;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float o = wv::shfl_xor(mn, off);
        mn = (o < mn) ? o : mn;
      }
      const uint64_t lo = wv::ballot(a0 == mn), hi = wv::ballot(a1 == mn);
      const int bit = lo ? wv::ffs64(lo) : (64 + (wv::ffs64(hi) & 63));
      if (lane == 0) {
        const bool on = r0 + u < nrows;
        int *r = rec + u * QUAL_WORDS;
        r[0] = on ? s : 0; r[1] = on ? (2 * (r0 + u) + 1) : 0;
        r[5] = on ? (int)wv::f2u(mn) : 0; r[6] = on ? bit : 0; r[7] = on ? (w[u].crc_ok & 1) : 0;
      }
    }
    wv::wave_sync();
    // ---- the in-order sums: lane 3 u + c walks sum c of window u ----
    if (lane < QUAL_PACK * 3) {
      const float acc = quality_sum128<false>(term + lane * QUAL_TERM_STRIDE);
      const int u = lane / 3, c = lane - 3 * u;
      rec[u * QUAL_WORDS + 2 + c] = (r0 + u < nrows) ? (int)wv::f2u(acc) : 0;
    }
    wv::wave_sync();
    if (my_row < a.rows) *out = rec[lane];
    wv::wave_sync();   // (the next pack overwrites both areas)
  }
}

}  // namespace rfidk
