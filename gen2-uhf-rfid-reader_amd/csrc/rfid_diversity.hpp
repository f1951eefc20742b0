// rfid_diversity.hpp -- the diversity stage of the batched path: behind the statistics of a pass, one rfid_diversity per EPC window of
// every GROUP of M consecutive traces -- the M receive antennas of one reader session, recorded together.  The decoder's 128
// decisions are the best one receive channel allows; a tag too weak for every antenna alone fails its CRC everywhere, and all
// antennas' samples of that frame sit in the same pass.  Adding the antennas' decision values r_j before the sign is taken is
// maximum-ratio combining (the weights are conj(h_est): equal noise power on every antenna) and gains 10 log10 M dB.  No new signal
// processing per member: each member's own window, dc_est, T, index and h_est, the decoder's two half-bit associations, its sign
// chain and its CRC.  No counterpart in the reference.  A combined frame is never counted as a read: it is reported on its own.
//
// The definition (include/rfid_mi355x.h, rfid_diversity) is in binary32, one rounding per operation, the members added in ascending
// order: a record is a function of the input alone.  The shape:
//   fetch    a persistent grid of single-wave workgroups over (group, block of DIV_ROWS = 8 table rows).  Lane 8 u + m holds member m
//            of row u of the block: ONE window record and ONE result record per lane, all 64 in flight together, whatever M is --
//            a lane that held a row's records of all members would carry 8 x 13 registers indexed by a run-time m.  The anchor's
//            start comes from lane 8 u by a shuffle; a ballot of `present` and one of `read` then hold every row's two member
//            masks as byte u, and the row's lowest reader's frame is four shuffles away.  Lane 8 u owns the row's record.
//   combine  one ballot finds the (row, member) pairs to add up: the present members of the rows nobody read and more than one
//            member heard.  They are taken in lane order -- row by row, members ascending -- one after the other: the member's
//            1 370 samples are staged DC-free in LDS (10 960 B: s is all the LDS holds, nothing is searched), each lane gathers
//            decisions lane and lane + 64 with that member's T, index and h_est and adds the two values to two accumulators in
//            registers; the loads of the NEXT pair (44 registers) are in flight meanwhile, as lengths_kernel has it.  A block
//            without such a row costs one round trip.
//   finish   behind a row's last member: epc_sign_chain over the accumulators' signs, the decoder's CRC-16 (epc_crc_holds' form,
//            keeping the two words it compares), a wave minimum of |acc| and the first lane that holds it by ballot -- among
//            j < 64 first -- as quality_kernel has it.
//   store    every row before the anchor's cut-off is written, rows behind it are zeroed; the first block writes nrows[g].
//   diversity_one_kernel   the same device functions on spans a caller holds, all members present.
// A window is never read behind its trace's own length (stage_span_last): the gate hands out whole windows, so this holds nothing.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int DIV_MAX = RFID_DIVERSITY_MAX_MEMBERS;
constexpr int DIV_SLACK = RFID_DIVERSITY_SLACK;
constexpr int DIV_ROWS = 8;                           // table rows per workgroup and step: lane 8 u + m is member m of row u
constexpr int DIV_LOADS = (EPC_WIN + 63) / 64;        // loads per lane and window
constexpr int DIV_WGS_PER_CU = 8;                     // most single-wave workgroups of a launch, per compute unit
constexpr float DIV_T_LO = 4.95f, DIV_T_HI = 5.05f;   // the decoder's own candidates: 4.94999981 .. 5.05000019
static_assert(sizeof(rfid_diversity) == 64, "rfid_diversity is sixteen words");
static_assert(DIV_MAX == 8 && DIV_ROWS * DIV_MAX == 64, "a lane per (row, member)");

// the window's samples i = lane + 64 k from src[min(i, last)]; last < 0: nothing to read
RFID_DEVICE void diversity_load(const float2 *src, int last, float2 (&v)[DIV_LOADS], int lane) {
#pragma unroll
  for (int k = 0; k < DIV_LOADS; ++k) {
    const int i = lane + 64 * k;
    v[k] = (i < EPC_WIN && last >= 0) ? src[(i < last) ? i : last] : make_float2(0.0f, 0.0f);
  }
}

// ... as s = in[i] - dc_est (gate_impl.cc:175-176) into LDS
RFID_DEVICE void diversity_stage(const float2 (&v)[DIV_LOADS], float dcr, float dci, float2 *s, int lane) {
#pragma unroll
  for (int k = 0; k < DIV_LOADS; ++k) {
    const int i = lane + 64 * k;
    if (i < EPC_WIN) s[i] = make_float2(v[k].x - dcr, v[k].y - dci);
  }
}

struct DivAcc {          // decisions lane and lane + 64 of the row in hand; h_sq the same in every lane
  float a0, a1, h_sq;
};

// one member's decision values r_j (as epc_decision forms them) onto the accumulators.  s: its staged window (visible to the wave);
// T, index, hre, him: its result's; first: the row's first present member
RFID_DEVICE void diversity_add(const float2 *s, float T, int index, float hre, float him, bool first, DivAcc &acc, int lane) {
  const float fidx = (float)index, nhim = -him;
  float2 pa, qa, pb, qb;
  epc_gather(s, T, fidx, lane, pa, qa, pb, qb);
  const float r0 = (pa.x - qa.x) * hre - (pa.y - qa.y) * nhim;
  const float r1 = (pb.x - qb.x) * hre - (pb.y - qb.y) * nhim;
  const float hh = hre * hre + him * him;
  if (first) { acc.a0 = r0; acc.a1 = r1; acc.h_sq = 0.0f; }
  else { acc.a0 = acc.a0 + r0; acc.a1 = acc.a1 + r1; }
  acc.h_sq = acc.h_sq + hh;
}

struct DivFound {        // (the same in every lane)
  int pass, rcvd, calc, weakest;
  float margin, h_sq;
  uint32_t f[4];
};

RFID_DEVICE DivFound diversity_finish(const DivAcc &acc, int lane) {
  DivFound r;
  uint64_t b0, b1;
  epc_sign_chain(acc.a0 > 0.0f, acc.a1 > 0.0f, b0, b1);
  r.f[0] = (uint32_t)b0; r.f[1] = (uint32_t)(b0 >> 32); r.f[2] = (uint32_t)b1; r.f[3] = (uint32_t)(b1 >> 32);
  // ---- check_crc (:401-445) as epc_crc_holds has it, the two words kept ----
  unsigned x = 0;
  if ((b0 >> lane) & 1ull) x ^= g_crc16.c[lane];
  if (lane < 48 && ((b1 >> lane) & 1ull)) x ^= g_crc16.c[lane + 64];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x ^= wv::shfl_xor(x, off);
  r.calc = (int)((~(x ^ (unsigned)g_crc16.k)) & 0xFFFFu);
  unsigned rcvd = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) rcvd |= (unsigned)((b1 >> (48 + i)) & 1ull) << (15 - i);
  r.rcvd = (int)rcvd;
  r.pass = (r.calc == r.rcvd) ? 1 : 0;
  // ---- min |acc_j| and the lowest j that attains it ----
  const float m0 = __builtin_fabsf(acc.a0), m1 = __builtin_fabsf(acc.a1);
  float mn = (m1 < m0) ? m1 : m0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = wv::shfl_xor(mn, off);
    mn = (o < mn) ? o : mn;
  }
  const uint64_t lo = wv::ballot(m0 == mn), hi = wv::ballot(m1 == mn);
  r.weakest = lo ? wv::ffs64(lo) : (64 + (wv::ffs64(hi) & 63));
  r.margin = mn;
  r.h_sq = acc.h_sq;
  return r;
}

// a combined frame into the record of its row
RFID_DEVICE void diversity_fill(rfid_diversity &rec, const DivFound &f) {
  rec.flags |= f.pass ? 2 : 0;
  rec.frame[0] = f.f[0]; rec.frame[1] = f.f[1]; rec.frame[2] = f.f[2]; rec.frame[3] = f.f[3];
  rec.crc_rcvd = f.rcvd; rec.crc_calc = f.calc;
  rec.h_sq = f.h_sq; rec.margin_min = f.margin; rec.weakest = f.weakest;
}

RFID_DEVICE void diversity_clear(rfid_diversity &rec) {
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.present = 0; rec.reads = 0;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
  rec.crc_rcvd = 0; rec.crc_calc = 0; rec.h_sq = 0.0f; rec.margin_min = 0.0f; rec.weakest = 0; rec.reserved_ = 0;
}

// what a row's member masks make of it: read by some (1), lone (4), or to combine (0)
RFID_DEVICE int diversity_class(int present, int reads) {
  return reads ? 1 : ((wv::popc64((uint64_t)present) < 2) ? 4 : 0);
}

struct DivArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp); p.n_streams = groups x members
  int members;                      // M: group g is traces g M .. g M + M - 1, member 0 the anchor
  int groups;
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / DIV_ROWS)
  const int64_t *lens;              // [n_streams] raw samples of every trace of the pass, or nullptr: n_dec for all
  int64_t n_dec;                    // matched-filter outputs of the pass's longest possible trace
  rfid_diversity *table;            // [groups][rows]
  int *nrows;                       // [groups]: the anchor's EPC windows before its cut-off (n_windows_used / 2)
};

RFID_KERNEL(64) void diversity_kernel(DivArgs a) {
  RFID_SHARED float2 s[EPC_WIN];
  const int lane = wv::lane_id();
  const int u = lane >> 3, m = lane & (DIV_MAX - 1), lane0 = lane & ~(DIV_MAX - 1);
  const int64_t n_items = (int64_t)a.groups * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int g = (int)(it / a.blocks);
    const int r0 = (int)(it - (int64_t)g * a.blocks) * DIV_ROWS;
    const int t0 = g * a.members;
    const int nrows = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, t0) >> 1;      // seq = 2 row + 1 < nw of the anchor
    if (r0 == 0 && lane == 0) a.nrows[g] = nrows;
    const int my_row = r0 + u;
    const bool mine = m == 0 && my_row < a.rows;               // (this lane stores a row)
    const bool on = m < a.members && my_row < nrows;
    const int k = 2 * my_row + 1;
    rfid_diversity rec;
    diversity_clear(rec);
    if (r0 < nrows) {
      // ---- every lane its own (row, member): window and result, all of the block in flight together ----
      const int trace = t0 + (on ? m : 0);
      int start = 0, index = 0, type = 0, crc_ok = 0;
      float dcr = 0.0f, dci = 0.0f, T = 0.0f, hre = 0.0f, him = 0.0f;
      uint32_t f0 = 0u, f1 = 0u, f2 = 0u, f3 = 0u;
      bool inside = false;                                     // window k lies before this member's own cut-off
      if (on) {
        inside = k < stage_windows(a.p.wcount, a.p.stats, a.p.wmax, trace);
        if (inside) {
          const rfid_window *wd = a.p.wtab + ((int64_t)trace * a.p.wmax + k);
          const rfid_decode_result *rs = a.p.res + ((int64_t)trace * a.p.wmax + k);
          start = wd->start; dcr = wd->dc_re; dci = wd->dc_im;
          type = rs->type; index = rs->index; hre = rs->h_re; him = rs->h_im; T = rs->T; crc_ok = rs->crc_ok;
          f0 = rs->bits[0]; f1 = rs->bits[1]; f2 = rs->bits[2]; f3 = rs->bits[3];
        }
      }
      const int start0 = wv::shfl(start, lane0);
      const int64_t apart = (int64_t)start - (int64_t)start0;
      const bool near = apart >= -(int64_t)DIV_SLACK && apart <= (int64_t)DIV_SLACK;
      const bool present = on && (m == 0 || (inside && type == RFID_DECODE_EPC && near));
      const bool read = present && inside && type == RFID_DECODE_EPC && crc_ok == 1;    // (a read, as stage_fetch has it)
      const uint64_t pm = wv::ballot(present), rm = wv::ballot(read);
      const int my_present = (int)((pm >> lane0) & 0xFFull), my_reads = (int)((rm >> lane0) & 0xFFull);
      const int cls = diversity_class(my_present, my_reads);
      // the frame of the row's lowest reader (this lane's own where there is none: unused)
      const int from = my_reads ? (lane0 + wv::ffs64((uint64_t)my_reads)) : lane;
      const uint32_t g0 = (uint32_t)wv::shfl((int)f0, from), g1 = (uint32_t)wv::shfl((int)f1, from);
      const uint32_t g2 = (uint32_t)wv::shfl((int)f2, from), g3 = (uint32_t)wv::shfl((int)f3, from);
      if (on && m == 0) {
        rec.stream = t0; rec.seq = k; rec.start = start; rec.flags = cls; rec.present = my_present; rec.reads = my_reads;
        if (cls == 1) { rec.frame[0] = g0; rec.frame[1] = g1; rec.frame[2] = g2; rec.frame[3] = g3; }
      }
      // ---- the (row, member) pairs to add up, in lane order; the loads of the next one are in flight meanwhile ----
      uint64_t todo = wv::ballot(present && cls == 0);
      float2 v[DIV_LOADS];
      int n_last = -1;
      if (todo) {
        const int nx = wv::ffs64(todo), nt = t0 + (nx & (DIV_MAX - 1)), n_start = wv::readlane(start, nx);
        n_last = stage_span_last(stage_extent(a.lens, a.n_dec, nt), n_start, EPC_WIN);
        diversity_load(a.p.y + (int64_t)nt * a.p.y_stride + n_start, n_last, v, lane);
      }
      DivAcc acc;
      acc.a0 = acc.a1 = acc.h_sq = 0.0f;
      while (todo) {
        const int lead = wv::ffs64(todo);
        todo &= todo - 1ull;
        diversity_stage(v, wv::readlane(dcr, lead), wv::readlane(dci, lead), s, lane);
        wv::wave_sync();
        const int nx = wv::ffs64(todo);                        // (64: none)
        if (todo) {
          const int nt = t0 + (nx & (DIV_MAX - 1)), n_start = wv::readlane(start, nx);
          n_last = stage_span_last(stage_extent(a.lens, a.n_dec, nt), n_start, EPC_WIN);
          diversity_load(a.p.y + (int64_t)nt * a.p.y_stride + n_start, n_last, v, lane);
        }
        diversity_add(s, wv::readlane(T, lead), wv::readlane(index, lead), wv::readlane(hre, lead), wv::readlane(him, lead),
                      (lead & (DIV_MAX - 1)) == 0, acc, lane);       // (the anchor is always present: a row's first)
        if ((nx >> 3) != (lead >> 3)) {                        // the row's last member
          const DivFound f = diversity_finish(acc, lane);
          if (lane == (lead & ~(DIV_MAX - 1))) diversity_fill(rec, f);
        }
        wv::wave_sync();   // (the next member overwrites the window)
      }
    }
    if (mine) a.table[(int64_t)g * a.rows + my_row] = rec;     // (behind the cut-off: zeros)
  }
}

// ---- caller-supplied spans (rfid_diversity_window): the same staging, sums and finish, one wave; spans: [members][EPC_WIN], DC-free ----
RFID_KERNEL(64) void diversity_one_kernel(const float2 *spans, int members, const rfid_decode_result *res, rfid_diversity *out) {
  RFID_SHARED float2 s[EPC_WIN];
  const int lane = wv::lane_id();
  const bool on = lane < members;
  const rfid_decode_result *rs = res + (on ? lane : 0);
  const bool read = on && rs->crc_ok == 1;
  const uint64_t rm = wv::ballot(read);
  rfid_diversity rec;
  diversity_clear(rec);
  rec.present = (1 << members) - 1;
  rec.reads = (int)(rm & 0xFFull);
  rec.flags = diversity_class(rec.present, rec.reads);
  if (rec.flags == 1) {
    const rfid_decode_result *lowest = res + wv::ffs64(rm);
    rec.frame[0] = lowest->bits[0]; rec.frame[1] = lowest->bits[1]; rec.frame[2] = lowest->bits[2]; rec.frame[3] = lowest->bits[3];
  } else if (rec.flags == 0) {
    DivAcc acc;
    acc.a0 = acc.a1 = acc.h_sq = 0.0f;
    float2 v[DIV_LOADS];
    diversity_load(spans, EPC_WIN - 1, v, lane);
    for (int mb = 0; mb < members; ++mb) {
      diversity_stage(v, 0.0f, 0.0f, s, lane);                 // (DC-free already)
      wv::wave_sync();
      if (mb + 1 < members) diversity_load(spans + (int64_t)(mb + 1) * EPC_WIN, EPC_WIN - 1, v, lane);
      diversity_add(s, res[mb].T, res[mb].index, res[mb].h_re, res[mb].h_im, mb == 0, acc, lane);
      wv::wave_sync();
    }
    diversity_fill(rec, diversity_finish(acc, lane));
  }
  if (lane == 0) *out = rec;
}

}  // namespace rfidk
