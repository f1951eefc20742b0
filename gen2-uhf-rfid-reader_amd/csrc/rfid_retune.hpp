// rfid_retune.hpp -- the retune stage of the batched path: behind the statistics of a pass, one rfid_retune per EPC window before the
// TERMINATED cut-off.  A window whose CRC-16 failed is decoded again with the half-bit period T searched over the whole tolerance
// Gen2 allows a tag's backscatter link frequency at this link setting (40 kHz +- 4 %): 81 candidates over 5.0 +- 4 % samples, where
// the decoder (tag_decoder_impl.cc:150-166) searches 20 over +- 1 %.  A tag further off than about 1 % fails every CRC and is
// absent from everything else a pass reports; three reversed decisions (the repair stage) do not undo a sampling comb that walks
// off the frame.  No counterpart in the reference.  A retuned frame is never counted as a read: it is reported on its own.
//
// The definition (include/rfid_mi355x.h, rfid_retune) is in binary32, one rounding per operation, every sum in order from 0.0f: a
// record is a function of the input alone.  The shape:
//   span     a slow tag's frame ends up to 38 samples behind the gate's 1 370-sample window, so a failed window is staged as
//            RFID_RETUNE_SPAN = 1408 = 22 x 64 samples from its start -- never behind the trace's own last sample (`last`: the
//            samples of a row behind the trace's length are not defined) -- as s = y - dc_est (float2) and p = |s|^2 (float) in
//            LDS: 11 264 + 5 632 = 16 896 bytes per single-wave workgroup, nine of them per compute unit's 160 KB.
//   search   lane l walks candidates t = l and l + 64 (81 = 64 + 17: the second walk keeps 17 lanes busy): 256 gathers of p each, a
//            chain of dependent additions (the sum is in order), so a failed window costs 81 x 256 gathers against the decoder's
//            20 x 256 -- in two walks of 256 steps, where the decoder's three windows per wave take one.
//            LDS layout: p plain, one word per sample, no padding.  The gathers are ds_read_b32 (32 banks of 4 bytes, conflicts
//            counted within each half of the wave).  At step i the 32 lanes of a half read p[(int)(i T_t + idx_t)] with T_t 0.005
//            apart: a run of at most (i + 13) x 0.155 <= 42 consecutive words that rises with the lane -- lanes on the same word are
//            served by one broadcast, and a run of up to 32 consecutive words lies in 32 different banks.  Only behind step 193 is
//            the run longer than 32 words, and then at most 10 of its words share a bank with another: a two-way conflict on some
//            of the last 62 steps of 256, none before.  Padding or swizzling p could not do better than that, and would put an
//            address computation on every gather.  s is gathered 4 + 6 times per window: its layout does not matter.
//   argmax   the energies are sums of squares, >= +0: their bit patterns order as the values do.  One wave maximum over the bit
//            patterns, then the first lane that holds it by ballot, t < 64 before t >= 64: the FIRST maximum, as the decoder's
//            std::max_element.
//   decide   h from the six preamble ones at the new T, the decoder's 128 decisions, sign chain and CRC through the device
//            functions the decoder kernels use themselves (rfid_kernels.hpp: epc_index_a / _b, epc_decision, epc_sign_chain,
//            epc_crc_holds).
//   retune_kernel   a persistent grid of single-wave workgroups over (trace, block of RET_ROWS table rows), one row per lane of the
//            first eight: stage_windows for the cut-off, every lane fetches its own row's window and result record, one ballot
//            finds the failed rows.  They are taken one after the other, as repair_kernel does -- a search is a chain of wave
//            operations over one span in LDS -- so blocks are short; the 22 loads per lane of the NEXT failed row are in flight
//            during a search (44 registers: with nine waves per compute unit there is room).  A block without a failed row costs
//            one round trip.  Every row before the cut-off is written, rows behind it are zeroed; the first block writes nrows[s].
//   retune_one_kernel   the same device functions on one span a caller holds.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int RET_SPAN = RFID_RETUNE_SPAN;
constexpr int RET_CAND = RFID_RETUNE_CANDIDATES;
constexpr int RET_LOADS = RET_SPAN / 64;  // loads per lane and span
constexpr int RET_ROWS = 8;               // table rows per workgroup and step, one per lane of the first eight
constexpr int RET_WGS_PER_CU = 8;         // most single-wave workgroups of a launch, per compute unit
constexpr int RET_WORDS = (int)(sizeof(rfid_retune) / sizeof(int));
constexpr float RET_T_LO = 4.8f, RET_T_HI = 5.2f;      // 5.0 -+ 4 %
static_assert(sizeof(rfid_retune) == 64 && RET_WORDS == 16, "rfid_retune is sixteen words");
static_assert(RET_SPAN == 64 * RET_LOADS && RET_SPAN >= EPC_WIN, "whole loads per lane");
static_assert(RET_CAND > 64 && RET_CAND <= 128, "two candidates per lane");
// the furthest index of the search: sync offset 14, 13 + 255 half-bits of 5.2 samples (14 + 268 x 5.2 = 1407.6)
static_assert((N_SYNC - 1) + 268 * 5.2 < RET_SPAN, "the span holds every index");

// candidate t of the grid
RFID_DEVICE float ret_T(int t) { return RET_T_LO + (float)t * ((RET_T_HI - RET_T_LO) / (float)(RET_CAND - 1)); }
// (never reached with a sync offset in 0 .. 14: an index stays inside the LDS arrays whatever a caller's record says)
RFID_DEVICE int ret_at(int i) { return (i < 0) ? 0 : ((i > RET_SPAN - 1) ? (RET_SPAN - 1) : i); }

// the span's samples i = lane + 64 k from src[min(i, last)]; last < 0: nothing to read
RFID_DEVICE void retune_load(const float2 *src, int last, float2 (&v)[RET_LOADS], int lane) {
#pragma unroll
  for (int k = 0; k < RET_LOADS; ++k) {
    const int i = lane + 64 * k;
    v[k] = (last >= 0) ? src[(i < last) ? i : last] : make_float2(0.0f, 0.0f);
  }
}

// ... as s = in[i] - dc_est (gate_impl.cc:175-176) and p = std::norm of it into LDS
RFID_DEVICE void retune_stage(const float2 (&v)[RET_LOADS], float dcr, float dci, float2 *s, float *p, int lane) {
#pragma unroll
  for (int k = 0; k < RET_LOADS; ++k) {
    const int i = lane + 64 * k;
    const float re = v[k].x - dcr, im = v[k].y - dci;
    s[i] = make_float2(re, im);
    p[i] = re * re + im * im;
  }
}

struct RetuneFound {     // (the same in every lane)
  int t, pass, clamped;
  float T, h_re, h_im, energy;
  uint32_t f[4];
};

struct RetuneCrc { unsigned lo, hi, k; };      // what a lane keeps of the CRC table: c[lane], c[lane + 64], k
RFID_DEVICE RetuneCrc retune_crc(int lane) {
  RetuneCrc c;
  c.lo = g_crc16.c[lane]; c.hi = (lane < 48) ? g_crc16.c[lane + 64] : 0u; c.k = g_crc16.k;
  return c;
}

// the decoder's energy metric (tag_decoder_impl.cc:150-166) of one candidate: 256 gathers, summed in order
RFID_DEVICE float retune_energy(const float *p, float T, float fidx) {
  float e = 0.0f;
#pragma unroll 16
  for (int i = 0; i < 256; ++i) e = e + p[ret_at(wv::f2i((float)i * T + fidx))];
  return e;
}

// s, p: the staged span (visible to the wave); m: the sync offset; last: the span's last own sample
RFID_DEVICE RetuneFound retune_search(const float2 *s, const float *p, int m, int last, const RetuneCrc &crc, int lane) {
  const float fm = (float)m;
  // ---- the grid: candidates lane and lane + 64 ----
  const bool two = lane + 64 < RET_CAND;
  const float T0 = ret_T(lane), T1 = ret_T(lane + 64);
  const float e0 = retune_energy(p, T0, fm + 13.0f * T0);
  float e1 = 0.0f;
  if (two) e1 = retune_energy(p, T1, fm + 13.0f * T1);
  // ---- the first maximum ----
  const unsigned k0 = wv::f2u(e0), k1 = two ? wv::f2u(e1) : 0u;
  unsigned mx = (k1 > k0) ? k1 : k0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned o = wv::shfl_xor(mx, off);
    mx = (o > mx) ? o : mx;
  }
  const uint64_t lo = wv::ballot(k0 == mx), hi = wv::ballot(two && k1 == mx);
  const int t = lo ? wv::ffs64(lo) : (64 + (wv::ffs64(hi) & 63));
  RetuneFound r;
  r.t = t;
  r.energy = wv::readlane((t < 64) ? e0 : e1, t & 63);
  const float T = ret_T(t), fidx = fm + 13.0f * T, T2 = 2.0f * T;
  r.T = T;
  // ---- h_est at the new T: the preamble's six ones (TAG_PREAMBLE, tag_decoder_impl.cc:78-103), left to right ----
  float cre = 0.0f, cim = 0.0f;
  const int ones[6] = {0, 1, 3, 6, 10, 11};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float2 v = s[ret_at(wv::f2i(fm + (float)ones[k] * T))];
    cre = cre + v.x;
    cim = cim + v.y;
  }
  r.h_re = wv::fdiv(cre, 6.0f);
  r.h_im = wv::fdiv(cim, 6.0f);
  const float nhim = -r.h_im;
  // ---- the decoder's decisions, sign chain and CRC ----
  const int ia0 = epc_index_a(lane, T2, fidx), ib0 = epc_index_b(lane, T, fidx);
  const int ia1 = epc_index_a(lane + 64, T2, fidx), ib1 = epc_index_b(lane + 64, T, fidx);
  const bool cur0 = epc_decision(s[ret_at(ia0)], s[ret_at(ib0)], r.h_re, nhim);
  const bool cur1 = epc_decision(s[ret_at(ia1)], s[ret_at(ib1)], r.h_re, nhim);
  uint64_t b0, b1;
  epc_sign_chain(cur0, cur1, b0, b1);
  r.f[0] = (uint32_t)b0; r.f[1] = (uint32_t)(b0 >> 32); r.f[2] = (uint32_t)b1; r.f[3] = (uint32_t)(b1 >> 32);
  r.pass = epc_crc_holds(b0, b1, crc.lo, crc.hi, crc.k, lane) ? 1 : 0;
  // ---- was an index held at `last`?  A walk's indices rise: its last one is its largest; the preamble's lie before the decisions' ----
  int far = wv::f2i(255.0f * T0 + (fm + 13.0f * T0));
  if (two) { const int w = wv::f2i(255.0f * T1 + (fm + 13.0f * T1)); far = (w > far) ? w : far; }
  far = (ib0 > far) ? ib0 : far;
  far = (ib1 > far) ? ib1 : far;
  far = (ia1 > far) ? ia1 : far;
  r.clamped = wv::ballot(far > last) ? 1 : 0;
  return r;
}

// a found frame into the record of its row
RFID_DEVICE void retune_fill(rfid_retune &rec, const RetuneFound &f) {
  rec.flags |= (f.pass ? 2 : 0) | (f.clamped ? 4 : 0);
  rec.t_index = f.t; rec.T = f.T; rec.h_re = f.h_re; rec.h_im = f.h_im; rec.energy = f.energy;
  rec.frame[0] = f.f[0]; rec.frame[1] = f.f[1]; rec.frame[2] = f.f[2]; rec.frame[3] = f.f[3];
}

RFID_DEVICE void retune_clear(rfid_retune &rec) {
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.t_index = 0;
  rec.T = 0.0f; rec.h_re = 0.0f; rec.h_im = 0.0f; rec.energy = 0.0f;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
  rec.reserved_[0] = rec.reserved_[1] = rec.reserved_[2] = 0;
}

struct RetArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / RET_ROWS)
  const int64_t *lens;              // [n_streams] raw samples of every trace of the pass, or nullptr: n_dec for all
  int64_t n_dec;                    // matched-filter outputs of the pass's longest possible trace
  rfid_retune *table;               // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

// the matched-filter outputs trace s holds (as gate_extent has it)
RFID_DEVICE int retune_extent(const RetArgs &a, int s) { return stage_extent(a.lens, a.n_dec, s); }

// the span's last own sample of a window that starts at `start` in a trace of n_dec outputs (-1: none)
RFID_DEVICE int retune_last(int n_dec, int start) { return stage_span_last(n_dec, start, RET_SPAN); }

RFID_KERNEL(64) void retune_kernel(RetArgs a) {
  RFID_SHARED float2 s[RET_SPAN];
  RFID_SHARED float p[RET_SPAN];
  const int lane = wv::lane_id();
  const RetuneCrc crc = retune_crc(lane);
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int strm = (int)(it / a.blocks);
    const int r0 = (int)(it - (int64_t)strm * a.blocks) * RET_ROWS;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, strm);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[strm] = nrows;
    const int my_row = r0 + lane;
    const bool mine = lane < RET_ROWS && my_row < a.rows;      // (this lane stores a row)
    const bool on = lane < RET_ROWS && my_row < nrows;
    const int k = 2 * my_row + 1;
    rfid_retune rec;
    retune_clear(rec);
    if (r0 < nrows) {
      // ---- every lane its own row: window and result, all rows of the block in flight together ----
      int start = 0, index = 0, type = 0, crc_ok = 0;
      float dcr = 0.0f, dci = 0.0f;
      if (on) {
        const rfid_window *wd = a.p.wtab + ((int64_t)strm * a.p.wmax + k);
        const int *rs = reinterpret_cast<const int *>(a.p.res + ((int64_t)strm * a.p.wmax + k));
        start = wd->start; dcr = wd->dc_re; dci = wd->dc_im;
        type = rs[0]; index = rs[1]; crc_ok = rs[10];
      }
      const bool ok = type == RFID_DECODE_EPC && crc_ok == 1;          // (a read, as stage_fetch has it)
      if (on) { rec.stream = strm; rec.seq = k; rec.start = start; rec.flags = ok ? 1 : 0; }
      // ---- the failed rows of the block, one after the other; the loads of the next one are in flight during a search ----
      const float2 *y = a.p.y + (int64_t)strm * a.p.y_stride;
      const int n_dec = retune_extent(a, strm);
      uint64_t todo = wv::ballot(on && !ok);
      float2 v[RET_LOADS];
      int n_start = 0, n_last = -1;
      if (todo) {
        n_start = wv::readlane(start, wv::ffs64(todo));
        n_last = retune_last(n_dec, n_start);
        retune_load(y + n_start, n_last, v, lane);
      }
      while (todo) {
        const int lead = wv::ffs64(todo);
        todo &= todo - 1ull;
        const int last = n_last;
        retune_stage(v, wv::readlane(dcr, lead), wv::readlane(dci, lead), s, p, lane);
        wv::wave_sync();
        if (todo) {
          n_start = wv::readlane(start, wv::ffs64(todo));
          n_last = retune_last(n_dec, n_start);
          retune_load(y + n_start, n_last, v, lane);
        }
        int m = wv::readlane(index, lead) - 65;                        // the decoder's sync (tag_decoder_impl.cc:107)
        m = (m < 0) ? 0 : ((m > N_SYNC - 1) ? (N_SYNC - 1) : m);
        const RetuneFound f = retune_search(s, p, m, last, crc, lane);
        if (lane == lead) retune_fill(rec, f);
        wv::wave_sync();   // (the next row overwrites both areas)
      }
    }
    if (mine) a.table[(int64_t)strm * a.rows + my_row] = rec;     // (behind the cut-off: zeros)
  }
}

// ---- one caller-supplied span (rfid_retune_window): the same staging and search, one wave; n: its samples (EPC_WIN .. RET_SPAN) ----
RFID_KERNEL(64) void retune_one_kernel(const float2 *span, int n, const rfid_decode_result *res, rfid_retune *out) {
  RFID_SHARED float2 s[RET_SPAN];
  RFID_SHARED float p[RET_SPAN];
  const int lane = wv::lane_id();
  const RetuneCrc crc = retune_crc(lane);
  const int *rs = reinterpret_cast<const int *>(res);
  rfid_retune rec;
  retune_clear(rec);
  rec.flags = rs[10] & 1;
  if (!rec.flags) {
    const int last = ((n > RET_SPAN) ? RET_SPAN : n) - 1;
    float2 v[RET_LOADS];
    retune_load(span, last, v, lane);
    retune_stage(v, 0.0f, 0.0f, s, p, lane);                           // (DC-free already)
    wv::wave_sync();
    int m = rs[1] - 65;
    m = (m < 0) ? 0 : ((m > N_SYNC - 1) ? (N_SYNC - 1) : m);
    const RetuneFound f = retune_search(s, p, m, last, crc, lane);
    retune_fill(rec, f);
  }
  if (lane == 0) *out = rec;
}

}  // namespace rfidk
