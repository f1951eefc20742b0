// rfid_stack.hpp -- the stack stage of the batched path: behind the statistics of a pass, one rfid_stack per EPC window before the
// TERMINATED cut-off.  Repair and retune work on one window alone, diversity needs several antennas, match needs the tag's EPC:
// a tag that is too weak in every round and that nobody knows is absent from all of them, however often an inventory session
// asked it for the same 128-bit frame.  Two failed windows that hold the same frame have strongly correlated decision values r_j
// (tag_decoder_impl.cc:171-190), windows that hold other frames, noise or collisions have uncorrelated ones: this stage finds, for
// every failed window, the failed windows near it whose r correlate with its own, adds their r_j before the sign is taken (each r
// carries its own conj(h_est): maximum-ratio combining over rounds, about 10 log10 K dB) and lets the decoder's CRC-16 decide
// whether the sum is a frame.  No counterpart in the reference.  A stacked frame is never counted as a read.
//
// The definition (include/rfid_mi355x.h, rfid_stack) is in binary32, one rounding per operation, every sum in order from 0.0f,
// every tie decided by the lower index: a record is a function of the input alone.  The shape:
//   stack_index_kernel   one wave per trace walks its table rows 64 at a time: a ballot of "not a verified read" and the popcount
//            of the lanes below give every failed row its ordinal f -- idx[f] = row, count[s] = F.  The same walk writes the
//            records that need nothing more: the reads (bit 0) and the zero rows behind the cut-off, and nrows[s].
//   stack_kernel   a persistent grid of single-wave workgroups over (trace, block of STK_BLOCK = 64 ordinals).  Lane l owns
//            ordinal 64 q + l: it fetches that row's window and result record, all of the block in flight together.
//     stage    row m = 0 .. n - 1 in turn: the wave gathers its 128 decisions (epc_gather, two per lane, formed by quality_rq: the
//            quality stage's own expression) into row m of a [64][128] LDS array, the NEXT row's four gathers issued before this
//            row's are used, as match_kernel has it.
//     load     lane l then takes row l into 128 registers, sixteen bytes at a time.
//     anchors  i = 0 .. n - 1 in turn: the anchor's r is read sixteen bytes at a time from an address all lanes share (a
//            broadcast, as in match_score), every lane forms s and a against its own row in one chain of 128 steps, one ballot of
//            the partner rule is the member mask.  With a partner, lanes j and j + 64 sum column j over the members in ascending
//            ordinal (the anchor in its place); epc_sign_chain and epc_crc_holds -- the decoder's own -- run over the sums, the
//            minimum and its lowest j as diversity_finish has them, sum |R_j| by quality_sum128 over 512 more bytes of LDS.
//            Lane i keeps the record.
//     store    every lane its own row's record.  A block with fewer than two failed rows costs one round trip and no LDS.
//   LDS layout: row m occupies words 128 m .. 128 m + 127 and is stored ROTATED by 4 m words: decision j of row m lies at word
//            (j + 4 m) mod 128 of its row.  The four kinds of access, by the bank rules of the LDS (64 banks of 4 bytes for
//            ds_read_b128, 32 for ds_read_b32 and every write; rows start 512 bytes apart: a bank depends on the word inside the
//            row alone):
//              stage   lanes write words (lane + 4 m) and (lane + 64 + 4 m) mod 128: each half-wave 32 consecutive words (a run
//                      that wraps at 128 keeps its banks apart, 128 being a multiple of 32): conflict-free.
//              load    the one access with a lane stride of a whole row.  Unrotated, all 64 lanes would read the same four banks:
//                      a 16-way conflict in each 16-lane group.  Rotated, lane l reads the 16-byte slot (k + l) mod 32 of its
//                      row in step k; a slot's banks are 4 (slot mod 16) .. + 3, and ds_read_b128 serves the lane groups
//                      {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: in each of them l mod 16 takes every value
//                      0 .. 15 once: sixteen different slots mod 16: conflict-free.  (A rotation by a multiple of four words keeps
//                      every 16-byte read aligned and whole: 128 is a multiple of 4.)
//              anchor  every lane reads slot (k + i) mod 32 of row i: one address, a broadcast.
//              column  lanes read word (j + 4 m) mod 128 of row m, j = lane and lane + 64: consecutive words again: conflict-free.
//   Registers: the row a lane holds is 128 VGPRs, beside them the two chains, the anchor's sixteen bytes in flight, the next row's
//            gathers and the record: 234 as compiled, no scratch.  32.5 KB of LDS allow four workgroups per compute unit, one wave
//            per SIMD, and a lone wave on a SIMD may use 512: the budget is not what limits residency, the LDS is
//            (STK_WGS_PER_CU = 4).
//   stack_one_kernel   the same device functions on up to 64 DC-free windows a caller holds.
// Departure from the sketch: the index kernel also writes the read and the zero rows, so that the block kernel stores failed rows
// only and a block without any costs one load of the trace's count.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_quality.hpp"

namespace rfidk {

constexpr int STK_BLOCK = RFID_STACK_BLOCK;
constexpr int STK_MAX_WINDOWS = RFID_STACK_MAX_WINDOWS;
constexpr int STK_WGS_PER_CU = 4;                     // most single-wave workgroups of the block kernel's launch, per compute unit: what the LDS holds
constexpr int STK_INDEX_WGS_PER_CU = 8;
constexpr float STK_T_LO = 4.95f, STK_T_HI = 5.05f;   // the decoder's own candidates: 4.94999981 .. 5.05000019
static_assert(sizeof(rfid_stack) == 64 && offsetof(rfid_stack, member_mask) == 24 && offsetof(rfid_stack, frame) == 48, "rfid_stack is sixteen words");
static_assert(STK_BLOCK == 64 && STK_MAX_WINDOWS == 64, "a lane per row of a block");

RFID_DEVICE void stack_clear(rfid_stack &rec) {
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.ordinal = 0; rec.n_partners = 0; rec.member_mask = 0ull;
  rec.sig_abs = 0.0f; rec.margin_min = 0.0f; rec.weakest = 0; rec.reserved_ = 0;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
}

// what a lane holds of its own row: where the window starts (in samples behind `base`), and what its gathers and decisions need
struct StkRow {
  int off, index;
  float dcr, dci, T, hre, him;
};

// where decision j of row m lies in the block's LDS array (words)
RFID_DEVICE int stack_word(int m, int j) { return 128 * m + ((j + 4 * m) & 127); }

// rows 0 .. n - 1 of the block into LDS: row m's decisions lane and lane + 64 from lane m's StkRow, the next row's gathers in flight
RFID_DEVICE void stack_stage(const float2 *base, const StkRow &w, int n, float *t, int lane) {
  float2 pa, qa, pb, qb;
  epc_gather(base + wv::readlane(w.off, 0), wv::readlane(w.T, 0), (float)wv::readlane(w.index, 0), lane, pa, qa, pb, qb);
  for (int m = 0; m < n; ++m) {
    float2 na = pa, nq = qa, nb = pb, nr = qb;
    if (m + 1 < n)
      epc_gather(base + wv::readlane(w.off, m + 1), wv::readlane(w.T, m + 1), (float)wv::readlane(w.index, m + 1), lane, na, nq, nb, nr);
    const float dcr = wv::readlane(w.dcr, m), dci = wv::readlane(w.dci, m), hre = wv::readlane(w.hre, m), him = wv::readlane(w.him, m);
    float r0, r1, q0, q1;
    quality_rq(pa, qa, dcr, dci, hre, him, r0, q0);
    quality_rq(pb, qb, dcr, dci, hre, him, r1, q1);
    t[stack_word(m, lane)] = r0;
    t[stack_word(m, lane + 64)] = r1;
    pa = na; qa = nq; pb = nb; qb = nr;
  }
}

// row `lane` of the LDS array into registers: own[j] = r^lane_j
RFID_DEVICE void stack_load(const float *t, float (&own)[128], int lane) {
  const float4 *row = reinterpret_cast<const float4 *>(t) + 32 * lane;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const float4 q = row[(k + lane) & 31];
    own[4 * k] = q.x; own[4 * k + 1] = q.y; own[4 * k + 2] = q.z; own[4 * k + 3] = q.w;
  }
}

// s = sum_j (x_j * own_j), a = sum_j |x_j * own_j| against anchor i's row: every product rounded, both sums in order from 0.0f
RFID_DEVICE void stack_correlate(const float *t, int i, const float (&own)[128], float &s, float &a) {
  const float4 *row = reinterpret_cast<const float4 *>(t) + 32 * i;
  s = 0.0f; a = 0.0f;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const float4 q = row[(k + i) & 31];
    const float p0 = q.x * own[4 * k], p1 = q.y * own[4 * k + 1], p2 = q.z * own[4 * k + 2], p3 = q.w * own[4 * k + 3];
    s = s + p0; a = a + __builtin_fabsf(p0);
    s = s + p1; a = a + __builtin_fabsf(p1);
    s = s + p2; a = a + __builtin_fabsf(p2);
    s = s + p3; a = a + __builtin_fabsf(p3);
  }
}

// the partner rule: s > 0 and s >= rho_min * a (one rounded product)
RFID_DEVICE bool stack_partner(float s, float a, float rho_min) {
  const float need = rho_min * a;
  return s > 0.0f && s >= need;
}

struct StkFound {        // (the same in every lane)
  int pass, weakest;
  float sig, margin;
  uint32_t f[4];
};

// the members' columns lane and lane + 64 summed in ascending ordinal, then the decoder's sign chain and CRC over the sums.
// t: the block's rows; ra: 128 more words of LDS
RFID_DEVICE StkFound stack_combine(const float *t, float *ra, uint64_t members, int lane) {
  float a0 = 0.0f, a1 = 0.0f;
  for (uint64_t mm = members; mm; mm &= mm - 1ull) {
    const int m = wv::ffs64(mm);
    a0 = a0 + t[stack_word(m, lane)];
    a1 = a1 + t[stack_word(m, lane + 64)];
  }
  StkFound r;
  uint64_t b0, b1;
  epc_sign_chain(a0 > 0.0f, a1 > 0.0f, b0, b1);
  r.f[0] = (uint32_t)b0; r.f[1] = (uint32_t)(b0 >> 32); r.f[2] = (uint32_t)b1; r.f[3] = (uint32_t)(b1 >> 32);
  r.pass = epc_crc_holds(b0, b1, g_crc16.c[lane], (lane < 48) ? g_crc16.c[lane + 64] : 0u, g_crc16.k, lane) ? 1 : 0;
  // ---- min |R_j| and the lowest j that attains it (as diversity_finish) ----
  const float m0 = __builtin_fabsf(a0), m1 = __builtin_fabsf(a1);
  float mn = (m1 < m0) ? m1 : m0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = wv::shfl_xor(mn, off);
    mn = (o < mn) ? o : mn;
  }
  const uint64_t lo = wv::ballot(m0 == mn), hi = wv::ballot(m1 == mn);
  r.weakest = lo ? wv::ffs64(lo) : (64 + (wv::ffs64(hi) & 63));
  r.margin = mn;
  // ---- sum |R_j| in the order of j ----
  ra[lane] = a0; ra[lane + 64] = a1;
  wv::wave_sync();
  r.sig = quality_sum128<true>(ra);
  wv::wave_sync();   // (the next anchor overwrites the sums)
  return r;
}

// a block of n >= 2 rows whose decisions lie in t: lane l < n gets the record fields of row l that the partners decide
RFID_DEVICE void stack_block(const float *t, float *ra, int n, float rho_min, rfid_stack &rec, int lane) {
  float own[128];
  stack_load(t, own, lane);
  for (int i = 0; i < n; ++i) {
    float s, a;
    stack_correlate(t, i, own, s, a);
    const uint64_t partners = wv::ballot(lane < n && lane != i && stack_partner(s, a, rho_min));
    const uint64_t members = partners | (1ull << i);
    if (lane == i) { rec.member_mask = members; rec.n_partners = wv::popc64(partners); }
    if (partners) {
      const StkFound f = stack_combine(t, ra, members, lane);
      if (lane == i) {
        rec.flags = 2 | (f.pass ? 4 : 0);
        rec.sig_abs = f.sig; rec.margin_min = f.margin; rec.weakest = f.weakest;
        rec.frame[0] = f.f[0]; rec.frame[1] = f.f[1]; rec.frame[2] = f.f[2]; rec.frame[3] = f.f[3];
      }
    }
  }
}

struct StkArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / STK_BLOCK): the most blocks of failed rows a trace can have
  float rho_min;
  int *idx;                         // [n_streams][rows]: the row of failed ordinal f
  int *count;                       // [n_streams]: F
  rfid_stack *table;                // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

RFID_KERNEL(64) void stack_index_kernel(StkArgs a) {
  const int lane = wv::lane_id();
  for (int strm = (int)blockIdx.x; strm < a.p.n_streams; strm += (int)gridDim.x) {
    const int nrows = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, strm) >> 1;      // seq = 2 row + 1 < nw
    int F = 0;
    for (int r0 = 0; r0 < a.rows; r0 += 64) {
      const int row = r0 + lane;
      const int k = 2 * row + 1;
      const bool on = row < nrows;
      bool read = false;
      rfid_stack rec;
      stack_clear(rec);
      if (on) {
        const rfid_decode_result *rs = a.p.res + ((int64_t)strm * a.p.wmax + k);
        read = rs->type == RFID_DECODE_EPC && rs->crc_ok == 1;      // (a read, as stage_fetch has it)
        if (read) {
          rec.stream = strm; rec.seq = k; rec.start = a.p.wtab[(int64_t)strm * a.p.wmax + k].start; rec.flags = 1; rec.ordinal = -1;
        }
      }
      const uint64_t failed = wv::ballot(on && !read);
      if (on && !read) a.idx[(int64_t)strm * a.rows + F + wv::popc64(failed & ((1ull << lane) - 1ull))] = row;
      else if (row < a.rows) a.table[(int64_t)strm * a.rows + row] = rec;             // (behind the cut-off: zeros)
      F += wv::popc64(failed);
    }
    if (lane == 0) { a.count[strm] = F; a.nrows[strm] = nrows; }
  }
}

RFID_KERNEL(64) void stack_kernel(StkArgs a) {
  RFID_SHARED float4 t4[STK_BLOCK * 32];
  RFID_SHARED float4 ra4[32];
  float *t = reinterpret_cast<float *>(t4), *ra = reinterpret_cast<float *>(ra4);
  const int lane = wv::lane_id();
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int strm = (int)(it / a.blocks);
    const int f0 = (int)(it - (int64_t)strm * a.blocks) * STK_BLOCK;
    int F = a.count[strm];
    if (F > a.rows) F = a.rows;
    int n = F - f0;
    if (n <= 0) continue;
    if (n > STK_BLOCK) n = STK_BLOCK;
    // ---- every lane its own row: window and result, all rows of the block in flight together ----
    const bool on = lane < n;
    int row = 0;
    StkRow w;
    w.off = 0; w.index = 0; w.dcr = w.dci = w.T = w.hre = w.him = 0.0f;
    rfid_stack rec;
    stack_clear(rec);
    if (on) {
      row = a.idx[(int64_t)strm * a.rows + f0 + lane];
      if (row < 0 || 2 * row + 1 >= a.p.wmax) row = 0;            // (never: the index kernel wrote it)
      const int k = 2 * row + 1;
      const rfid_window *wd = a.p.wtab + ((int64_t)strm * a.p.wmax + k);
      const rfid_decode_result *rs = a.p.res + ((int64_t)strm * a.p.wmax + k);
      w.off = wd->start; w.dcr = wd->dc_re; w.dci = wd->dc_im;
      w.index = rs->index; w.hre = rs->h_re; w.him = rs->h_im; w.T = rs->T;
      rec.stream = strm; rec.seq = k; rec.start = w.off; rec.ordinal = f0 + lane; rec.member_mask = 1ull << lane;
    }
    if (n >= 2) {
      stack_stage(a.p.y + (int64_t)strm * a.p.y_stride, w, n, t, lane);
      wv::wave_sync();
      stack_block(t, ra, n, a.rho_min, rec, lane);
      wv::wave_sync();   // (the next block overwrites the rows)
    }
    if (on) a.table[(int64_t)strm * a.rows + row] = rec;
  }
}

// ---- caller-supplied windows (rfid_stack_windows): the same staging and block functions, one wave; gated: [n][EPC_WIN], DC-free.
//      The windows whose own CRC held are reads (bit 0, ordinal -1); the others get their ordinals in the order given ----
RFID_KERNEL(64) void stack_one_kernel(const float2 *gated, const rfid_decode_result *res, int n_win, float rho_min, rfid_stack *out) {
  RFID_SHARED float4 t4[STK_BLOCK * 32];
  RFID_SHARED float4 ra4[32];
  RFID_SHARED int which[STK_BLOCK];
  float *t = reinterpret_cast<float *>(t4), *ra = reinterpret_cast<float *>(ra4);
  const int lane = wv::lane_id();
  const bool given = lane < n_win;
  const bool read = given && res[lane].crc_ok == 1;
  const uint64_t failed = wv::ballot(given && !read);
  const int n = wv::popc64(failed);
  if (given && !read) which[wv::popc64(failed & ((1ull << lane) - 1ull))] = lane;
  wv::wave_sync();
  rfid_stack rec;
  stack_clear(rec);
  if (read) { rec.flags = 1; rec.ordinal = -1; out[lane] = rec; }
  stack_clear(rec);
  const bool on = lane < n;
  int win = 0;
  StkRow w;
  w.off = 0; w.index = 0; w.dcr = w.dci = w.T = w.hre = w.him = 0.0f;
  if (on) {
    win = which[lane];
    const rfid_decode_result *rs = res + win;
    w.off = win * EPC_WIN; w.index = rs->index; w.hre = rs->h_re; w.him = rs->h_im; w.T = rs->T;      // (DC-free already)
    rec.ordinal = lane; rec.member_mask = 1ull << lane;
  }
  if (n >= 2) {
    stack_stage(gated, w, n, t, lane);
    wv::wave_sync();
    stack_block(t, ra, n, rho_min, rec, lane);
  }
  if (on) out[win] = rec;
}

}  // namespace rfidk
