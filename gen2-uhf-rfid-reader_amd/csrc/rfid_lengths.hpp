// rfid_lengths.hpp -- the lengths stage of the batched path: behind the statistics of a pass, one rfid_sized_frame per EPC window
// before the TERMINATED cut-off.  A tag answers an ACK with PC + EPC + CRC-16, and the first five PC bits give the EPC's length L in
// 16-bit words.  The decoder (tag_decoder_impl.cc:171-190, :401-445) takes every reply for 128 bits -- L = 6 -- so a tag with a
// 128- or a 64-bit EPC fails every CRC and is absent from everything else a pass reports, however cleanly it replied.  A window
// whose CRC-16 failed is read again here at the length its own PC announces: n = 32 + 16 L bits, L = 0 .. 8 but 6.  No new signal
// processing: the decoder's own T, index and h_est of the window, its two half-bit associations and its sign chain, continued past
// decision 127 where the frame is longer, and its CRC over n bits.  No counterpart in the reference.  A frame found here is never
// counted as a read: it is reported on its own.
//
// The definition (include/rfid_mi355x.h, rfid_sized_frame) is in binary32, one rounding per operation: a record is a function of
// the input alone.  The shape:
//   span     a frame of L = 7 or 8 ends behind the gate's 1 370-sample window, on the reader's carrier (which lasts 1 830 samples
//            after the ACK): the furthest half-bit of a 160-bit frame is at 79 + 319 x 5.05000019 = 1689.95 samples.  A failed
//            window is staged as RFID_LENGTHS_SPAN = 1728 = 27 x 64 samples from its start -- never behind the trace's own last
//            sample (`last`) -- as s = y - dc_est (float2) in LDS: 13 824 bytes per single-wave workgroup, eleven of them per compute
//            unit's 160 KB.  s is all the LDS holds: nothing is searched, so no |s|^2.  A frame of L < 6 lies inside the window: its
//            loads stop at sample 1 408 (22 per lane instead of 27).
//   decide   lanes take decisions j = lane, lane + 64 and lane + 128 (rfid_kernels.hpp: epc_index_a / _b, epc_decision): the third
//            group holds 32 lanes at L = 8, 16 at L = 7 and none below.  Bit j is (sign j differs from sign j - 1): the sign chain
//            runs over 160 decisions and a ballot holds 64, so it carries across three ballots -- the top sign of one into the
//            bottom of the next, as epc_sign_chain carries it across two.
//   CRC      CRC-16/CCITT is GF(2)-linear: register = K ^ XOR of what the set bits contribute, and what a bit contributes depends
//            only on the number of bits behind it.  One table by that distance and one constant per length (g_crc16_sized,
//            rfid_kernels.hpp) serve every n; a wave XOR-reduction as epc_crc_holds has it.
//   lengths_kernel   a persistent grid of single-wave workgroups over (trace, block of LEN_ROWS table rows), one row per lane of the
//            first eight: stage_windows for the cut-off, every lane fetches its own row's window and result record and reads L from
//            it, one ballot finds the rows to decode.  They are taken one after the other -- a decode is a chain of wave operations
//            over one span in LDS -- and the loads of the NEXT row are in flight meanwhile (54 registers), as retune_kernel has it.
//            A block without such a row costs one round trip.  Every row before the cut-off is written, rows behind it are zeroed;
//            the first block writes nrows[s].
//   lengths_one_kernel   the same device functions on one span a caller holds.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int LEN_SPAN = RFID_LENGTHS_SPAN;
constexpr int LEN_MAX_WORDS = RFID_LENGTHS_MAX_WORDS;
constexpr int LEN_OWN_WORDS = 6;                      // the decoder's own length: a 96-bit EPC
constexpr int LEN_LOADS = LEN_SPAN / 64;              // loads per lane and span
constexpr int LEN_LOADS_SHORT = (EPC_WIN + 63) / 64;  // ... of a frame that lies inside the window (L < 6)
constexpr int LEN_ROWS = 8;                           // table rows per workgroup and step, one per lane of the first eight
constexpr int LEN_WGS_PER_CU = 8;                     // most single-wave workgroups of a launch, per compute unit
constexpr float LEN_T_LO = 4.95f, LEN_T_HI = 5.05f;   // the decoder's own candidates: 4.94999981 .. 5.05000019
static_assert(sizeof(rfid_sized_frame) == 64, "rfid_sized_frame is sixteen words");
static_assert(LEN_SPAN == 64 * LEN_LOADS && LEN_SPAN >= EPC_WIN, "whole loads per lane");
static_assert(LEN_MAX_WORDS == Crc16Sized::MAX_WORDS && 32 + 16 * LEN_MAX_WORDS <= 3 * 64, "three decisions per lane");
// the furthest index: sync offset 14, the second sample of decision 159 (79 + 319 x 5.05000019 = 1689.95); of a frame inside the
// window: decision 111 (79 + 223 x 5.05000019 = 1205.2)
static_assert(65 + (N_SYNC - 1) + (2 * (32 + 16 * LEN_MAX_WORDS) - 1) * 5.0500002 < LEN_SPAN, "the span holds every index");
static_assert(65 + (N_SYNC - 1) + (2 * (32 + 16 * (LEN_OWN_WORDS - 1)) - 1) * 5.0500002 < EPC_WIN, "a short frame's loads hold every index");
static_assert(Crc16Sized().k[LEN_OWN_WORDS] == Crc16Table().k && Crc16Sized().d[111] == Crc16Table().c[0] && Crc16Sized().d[0] == Crc16Table().c[111],
              "at the decoder's own length: its table");

// (never reached with a result of the decoder's: an index stays inside the LDS array whatever a caller's record says)
RFID_DEVICE int len_at(int i) { return (i < 0) ? 0 : ((i > LEN_SPAN - 1) ? (LEN_SPAN - 1) : i); }

// L of a frame: its first five bits, the first the most significant (bits packed as rfid_decode_result::bits)
RFID_DEVICE int len_words(uint32_t w0) {
  int L = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) L |= (int)((w0 >> i) & 1u) << (4 - i);
  return L;
}
// does the stage decode a frame of L words?
RFID_DEVICE bool len_decodes(int L) { return L != LEN_OWN_WORDS && L <= LEN_MAX_WORDS; }
RFID_DEVICE int len_loads(int L) { return (L < LEN_OWN_WORDS) ? LEN_LOADS_SHORT : LEN_LOADS; }

// the first nl loads of the span's samples i = lane + 64 k from src[min(i, last)]; last < 0: nothing to read
RFID_DEVICE void lengths_load(const float2 *src, int last, int nl, float2 (&v)[LEN_LOADS], int lane) {
#pragma unroll
  for (int k = 0; k < LEN_LOADS; ++k) {
    const int i = lane + 64 * k;
    v[k] = (k < nl && last >= 0) ? src[(i < last) ? i : last] : make_float2(0.0f, 0.0f);
  }
}

// ... as s = in[i] - dc_est (gate_impl.cc:175-176) into LDS
RFID_DEVICE void lengths_stage(const float2 (&v)[LEN_LOADS], int nl, float dcr, float dci, float2 *s, int lane) {
#pragma unroll
  for (int k = 0; k < LEN_LOADS; ++k)
    if (k < nl) s[lane + 64 * k] = make_float2(v[k].x - dcr, v[k].y - dci);
}

struct SizedFound {      // (the same in every lane)
  int n, pass, clamped, rcvd, calc;
  uint32_t f[5];
};

// the bits j < n of the group of 64 that starts at j0
RFID_DEVICE uint64_t len_group_mask(int n, int j0) {
  const int k = n - j0;
  return (k >= 64) ? ~0ull : ((k <= 0) ? 0ull : ((1ull << k) - 1ull));
}

// s: the staged span (visible to the wave); L: the frame's EPC words (len_decodes); T, index, hre, him: the window's result;
// last: the span's last own sample
RFID_DEVICE SizedFound lengths_decide(const float2 *s, int L, float T, int index, float hre, float him, int last, int lane) {
  SizedFound r;
  const int n = 32 + 16 * L, m = n - 16;
  r.n = n;
  const float fidx = (float)index, T2 = 2.0f * T, nhim = -him;
  // ---- the decoder's decisions, three per lane, and its sign chain across the three ballots ----
  bool cur[3] = {false, false, false};
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const int j = lane + 64 * g;
    if (64 * g < n) {        // (the same in every lane: a group no decision falls into is not gathered)
      const float2 p = s[len_at(epc_index_a(j, T2, fidx))], q = s[len_at(epc_index_b(j, T, fidx))];
      cur[g] = j < n && epc_decision(p, q, hre, nhim);
    }
  }
  const uint64_t c0 = wv::ballot(cur[0]), c1 = wv::ballot(cur[1]), c2 = wv::ballot(cur[2]);
  const uint64_t b0 = (c0 ^ ((c0 << 1) | 1ull)) & len_group_mask(n, 0);
  const uint64_t b1 = (c1 ^ ((c1 << 1) | (c0 >> 63))) & len_group_mask(n, 64);
  const uint64_t b2 = (c2 ^ ((c2 << 1) | (c1 >> 63))) & len_group_mask(n, 128);
  r.f[0] = (uint32_t)b0; r.f[1] = (uint32_t)(b0 >> 32); r.f[2] = (uint32_t)b1; r.f[3] = (uint32_t)(b1 >> 32); r.f[4] = (uint32_t)b2;
  // ---- check_crc (:401-445) over bits 0 .. m - 1 against bits m .. n - 1: a set bit j contributes d[m - 1 - j] ----
  unsigned x = 0;
  const uint64_t bw[3] = {b0, b1, b2};
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const int j = lane + 64 * g;
    if (j < m && ((bw[g] >> lane) & 1ull)) x ^= g_crc16_sized.d[m - 1 - j];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x ^= wv::shfl_xor(x, off);
  r.calc = (int)((~(x ^ (unsigned)g_crc16_sized.k[L])) & 0xFFFFu);
  // (m is a multiple of 16: the sixteen bits lie in one ballot)
  const uint64_t top = (m < 64) ? b0 : ((m < 128) ? b1 : b2);
  const unsigned tail = (unsigned)(top >> (m & 63)) & 0xFFFFu;
  unsigned rcvd = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) rcvd |= ((tail >> i) & 1u) << (15 - i);
  r.rcvd = (int)rcvd;
  r.pass = (r.calc == r.rcvd) ? 1 : 0;
  // ---- was an index held at `last`?  They rise with j: the second sample of the last decision is the furthest ----
  r.clamped = (epc_index_b(n - 1, T, fidx) > last) ? 1 : 0;
  return r;
}

// a decoded frame into the record of its row
RFID_DEVICE void lengths_fill(rfid_sized_frame &rec, const SizedFound &f) {
  rec.flags |= (f.pass ? 2 : 0) | (f.clamped ? 4 : 0);
  rec.n_bits = f.n; rec.crc_rcvd = f.rcvd; rec.crc_calc = f.calc;
#pragma unroll
  for (int i = 0; i < 5; ++i) rec.frame[i] = f.f[i];
}

// what a failed window's record says of its length before anything is decoded
RFID_DEVICE void lengths_announce(rfid_sized_frame &rec, int L) {
  rec.words = L;
  if (L == LEN_OWN_WORDS) rec.flags |= 16;
  else if (L > LEN_MAX_WORDS) rec.flags |= 8;
}

RFID_DEVICE void lengths_clear(rfid_sized_frame &rec) {
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.words = 0; rec.n_bits = 0; rec.crc_rcvd = 0; rec.crc_calc = 0;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = rec.frame[4] = 0u;
  rec.reserved_[0] = rec.reserved_[1] = rec.reserved_[2] = 0;
}

struct LenArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / LEN_ROWS)
  const int64_t *lens;              // [n_streams] raw samples of every trace of the pass, or nullptr: n_dec for all
  int64_t n_dec;                    // matched-filter outputs of the pass's longest possible trace
  rfid_sized_frame *table;          // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

RFID_KERNEL(64) void lengths_kernel(LenArgs a) {
  RFID_SHARED float2 s[LEN_SPAN];
  const int lane = wv::lane_id();
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int strm = (int)(it / a.blocks);
    const int r0 = (int)(it - (int64_t)strm * a.blocks) * LEN_ROWS;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, strm);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[strm] = nrows;
    const int my_row = r0 + lane;
    const bool mine = lane < LEN_ROWS && my_row < a.rows;      // (this lane stores a row)
    const bool on = lane < LEN_ROWS && my_row < nrows;
    const int k = 2 * my_row + 1;
    rfid_sized_frame rec;
    lengths_clear(rec);
    if (r0 < nrows) {
      // ---- every lane its own row: window and result, all rows of the block in flight together ----
      int start = 0, index = 0, type = 0, crc_ok = 0, L = 0;
      float dcr = 0.0f, dci = 0.0f, T = 0.0f, hre = 0.0f, him = 0.0f;
      if (on) {
        const rfid_window *wd = a.p.wtab + ((int64_t)strm * a.p.wmax + k);
        const rfid_decode_result *rs = a.p.res + ((int64_t)strm * a.p.wmax + k);
        start = wd->start; dcr = wd->dc_re; dci = wd->dc_im;
        type = rs->type; index = rs->index; hre = rs->h_re; him = rs->h_im; T = rs->T; crc_ok = rs->crc_ok;
        L = len_words(rs->bits[0]);
      }
      const bool ok = type == RFID_DECODE_EPC && crc_ok == 1;          // (a read, as stage_fetch has it)
      if (on) {
        rec.stream = strm; rec.seq = k; rec.start = start; rec.flags = ok ? 1 : 0;
        if (!ok) lengths_announce(rec, L);
      }
      // ---- the rows to decode, one after the other; the loads of the next one are in flight meanwhile ----
      const float2 *y = a.p.y + (int64_t)strm * a.p.y_stride;
      const int n_dec = stage_extent(a.lens, a.n_dec, strm);
      uint64_t todo = wv::ballot(on && !ok && len_decodes(L));
      float2 v[LEN_LOADS];
      int n_last = -1, n_nl = 0;
      if (todo) {
        const int nx = wv::ffs64(todo), n_start = wv::readlane(start, nx);
        n_last = stage_span_last(n_dec, n_start, LEN_SPAN);
        n_nl = len_loads(wv::readlane(L, nx));
        lengths_load(y + n_start, n_last, n_nl, v, lane);
      }
      while (todo) {
        const int lead = wv::ffs64(todo);
        todo &= todo - 1ull;
        const int last = n_last;
        lengths_stage(v, n_nl, wv::readlane(dcr, lead), wv::readlane(dci, lead), s, lane);
        wv::wave_sync();
        if (todo) {
          const int nx = wv::ffs64(todo), n_start = wv::readlane(start, nx);
          n_last = stage_span_last(n_dec, n_start, LEN_SPAN);
          n_nl = len_loads(wv::readlane(L, nx));
          lengths_load(y + n_start, n_last, n_nl, v, lane);
        }
        const SizedFound f = lengths_decide(s, wv::readlane(L, lead), wv::readlane(T, lead), wv::readlane(index, lead),
                                            wv::readlane(hre, lead), wv::readlane(him, lead), last, lane);
        if (lane == lead) lengths_fill(rec, f);
        wv::wave_sync();   // (the next row overwrites the span)
      }
    }
    if (mine) a.table[(int64_t)strm * a.rows + my_row] = rec;     // (behind the cut-off: zeros)
  }
}

// ---- one caller-supplied span (rfid_length_window): the same staging and decisions, one wave; n: its samples (EPC_WIN .. LEN_SPAN) ----
RFID_KERNEL(64) void lengths_one_kernel(const float2 *span, int n, const rfid_decode_result *res, rfid_sized_frame *out) {
  RFID_SHARED float2 s[LEN_SPAN];
  const int lane = wv::lane_id();
  rfid_sized_frame rec;
  lengths_clear(rec);
  rec.flags = res->crc_ok & 1;
  if (!rec.flags) {
    const int L = len_words(res->bits[0]);
    lengths_announce(rec, L);
    if (len_decodes(L)) {
      const int last = ((n > LEN_SPAN) ? LEN_SPAN : n) - 1, nl = len_loads(L);
      float2 v[LEN_LOADS];
      lengths_load(span, last, nl, v, lane);
      lengths_stage(v, nl, 0.0f, 0.0f, s, lane);                         // (DC-free already)
      wv::wave_sync();
      const SizedFound f = lengths_decide(s, L, res->T, res->index, res->h_re, res->h_im, last, lane);
      lengths_fill(rec, f);
    }
  }
  if (lane == 0) *out = rec;
}

}  // namespace rfidk
