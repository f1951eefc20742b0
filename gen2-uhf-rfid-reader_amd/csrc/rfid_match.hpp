// rfid_match.hpp -- the match stage of the batched path: behind a pass, one rfid_match per EPC window before the TERMINATED cut-off.
// Repair, retune, lengths and diversity all DECODE a window whose CRC-16 failed: the frame must come out whole.  This stage DETECTS:
// a tag the pass already knows -- an entry of the same trace's inventory, or a frame of a list the caller supplies -- has a known
// reply of 128 bits, and a known reply is a known pattern of 128 signs.  Correlating the window's decision values r_j
// (tag_decoder_impl.cc:171-190) against that pattern is a matched filter over the whole frame: no single decision has to be right.
// No counterpart in the reference.  An attribution is never a read, and whether a score is one is the host's to say
// (rfid.batch.match_fields): the device reports the two best candidates, their scores and sum |r_j|.
//
// The definition (include/rfid_mi355x.h, rfid_match) is in binary32, one rounding per operation, every score an in-order sum from
// 0.0f, every tie decided by the lower index: a record is a function of the input alone.  The shape:
//   pattern  the decoder's chain is bit_j = c_j XOR c_(j-1) with c_(-1) = 1, so the one sign sequence that yields frame b is
//            c_j = 1 XOR b_0 XOR ... XOR b_j: a prefix XOR over 128 bits -- six shifts per 64-bit half and the carry of the lower half's
//            parity (match_pattern).  What is kept is the NEGATION mask, the prefix XOR itself: t_j = -r_j where its bit j is set.
//   score    the 128 r_j of the window in hand lie in LDS (512 bytes, r formed by quality_rq: the quality stage's own expression).
//            Lane l takes candidate 64 k + l of chunk k: its frame in four registers, its mask in four more, then j = 0 .. 127 in
//            order, the r_j read sixteen bytes at a time from an address all lanes share (a broadcast: no bank conflict), the sign
//            bit toggled by the mask's bit, one addition.  No lane's sum depends on another's: 64 candidates cost one chain of 128
//            additions.  A lane keeps the two best of its own candidates (they come in ascending index: the earlier one stays ahead
//            on equal scores), so inventories of more than 64 entries and lists are one loop over chunks.
//   best     behind the last chunk, one wave maximum over (score, then lower index) gives best; the lane that held it puts its own
//            second in its place and the same maximum gives second.  The order is total, so the result does not depend on how the
//            candidates were dealt to lanes and chunks.  dist_best and diff are popcounts over the frames / the masks.
//   sig_abs  quality_sum128<true> over the same LDS array: the quality stage's in-order sum, here over |r_j|.
//   match_kernel   a persistent grid of single-wave workgroups over (trace, block of MAT_ROWS = 8 table rows), one row per lane of
//            the first eight: stage_windows for the cut-off, every lane fetches its own row's window and result record, one ballot
//            finds the failed rows.  They are taken one after the other -- a search is one chain over one LDS array -- and the
//            gathers of the NEXT row (epc_gather: 8 registers) are in flight meanwhile, as lengths_kernel and repair_kernel have it.
//            A block without a failed row, or a trace without candidates, costs one round trip.  Every row before the cut-off is
//            written, rows behind it are zeroed; the first block writes nrows[s].
//   match_one_kernel   the same device functions on one span and one list a caller holds.
// Nothing is shared between workgroups, no atomics.  Only primitives both device environments offer.
#pragma once
#include "rfid_quality.hpp"

namespace rfidk {

constexpr int MAT_MAX_LIST = RFID_MATCH_MAX_LIST;
constexpr int MAT_ROWS = 8;                           // table rows per workgroup and step, one per lane of the first eight
constexpr int MAT_WGS_PER_CU = 8;                     // most single-wave workgroups of a launch, per compute unit
constexpr float MAT_T_LO = 4.95f, MAT_T_HI = 5.05f;   // the decoder's own candidates: 4.94999981 .. 5.05000019
static_assert(sizeof(rfid_match) == 64, "rfid_match is sixteen words");
static_assert(sizeof(rfid_tag_entry) == 48 && offsetof(rfid_tag_entry, frame) == 8, "an inventory entry's frame is words 2 .. 5");

// where a trace's candidate frames lie: frame i is the four words at f + i * stride
struct MatCands {
  const uint32_t *f;
  int stride;      // in words: 4 (a list), 12 (inventory entries)
  int n;
};

// the negation mask of a candidate frame: bit j set where c_j = 0, i.e. the prefix XOR b_0 ^ ... ^ b_j
RFID_DEVICE void match_pattern(const uint32_t (&f)[4], uint32_t (&n)[4]) {
  uint64_t p0 = (uint64_t)f[0] | ((uint64_t)f[1] << 32), p1 = (uint64_t)f[2] | ((uint64_t)f[3] << 32);
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) { p0 ^= p0 << sh; p1 ^= p1 << sh; }
  if (p0 >> 63) p1 = ~p1;      // (the parity of bits 0 .. 63 runs on into the upper half)
  n[0] = (uint32_t)p0; n[1] = (uint32_t)(p0 >> 32); n[2] = (uint32_t)p1; n[3] = (uint32_t)(p1 >> 32);
}

// (((0.0f + t_0) + t_1) + ...) + t_127, t_j = -r_j where bit j of the mask is set; r: the window's 128 decision values in LDS
RFID_DEVICE float match_score(const float4 *r, const uint32_t (&n)[4]) {
  float acc = 0.0f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float4 q = r[8 * w + k];
      const uint32_t m = n[w] >> (4 * k);
      acc = acc + wv::u2f(wv::f2u(q.x) ^ ((m & 1u) << 31));
      acc = acc + wv::u2f(wv::f2u(q.y) ^ (((m >> 1) & 1u) << 31));
      acc = acc + wv::u2f(wv::f2u(q.z) ^ (((m >> 2) & 1u) << 31));
      acc = acc + wv::u2f(wv::f2u(q.w) ^ (((m >> 3) & 1u) << 31));
    }
  }
  return acc;
}

// is candidate (so, io) ahead of (s, i)?  An index < 0: none.  The larger score, the lower index on equal scores
RFID_DEVICE bool match_ahead(float so, int io, float s, int i) { return io >= 0 && (i < 0 || so > s || (so == s && io < i)); }

// the wave's first by match_ahead, in every lane
RFID_DEVICE void match_wave_first(float &s, int &i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float so = wv::shfl_xor(s, off);
    const int io = wv::shfl_xor(i, off);
    if (match_ahead(so, io, s, i)) { s = so; i = io; }
  }
}

RFID_DEVICE void match_frame(const MatCands &c, int i, uint32_t (&f)[4]) {
  const uint32_t *g = c.f + (int64_t)i * c.stride;
  f[0] = g[0]; f[1] = g[1]; f[2] = g[2]; f[3] = g[3];
}

struct MatFound {        // (the same in every lane)
  int best, second, dist, diff;
  float s_best, s_second, sig;
  uint32_t f[4];
};

// r: the window's decision values (visible to the wave); c: the candidates, c.n >= 1; b: the window's decoded bits
RFID_DEVICE MatFound match_search(const float4 *r, const MatCands &c, const uint32_t (&b)[4], int lane) {
  MatFound m;
  m.sig = quality_sum128<true>(reinterpret_cast<const float *>(r));
  // ---- every lane the two best of its own candidates ----
  float s1 = 0.0f, s2 = 0.0f;
  int i1 = -1, i2 = -1;
  for (int base = 0; base < c.n; base += 64) {
    const int i = base + lane;
    if (i < c.n) {
      uint32_t f[4], n[4];
      match_frame(c, i, f);
      match_pattern(f, n);
      const float s = match_score(r, n);
      if (match_ahead(s, i, s1, i1)) { s2 = s1; i2 = i1; s1 = s; i1 = i; }
      else if (match_ahead(s, i, s2, i2)) { s2 = s; i2 = i; }
    }
  }
  // ---- the wave's best, then its second: the lane that held best puts its own second forward ----
  float sb = s1;
  int ib = i1;
  match_wave_first(sb, ib);
  float ss = (i1 == ib) ? s2 : s1;
  int is = (i1 == ib) ? i2 : i1;
  match_wave_first(ss, is);
  m.best = ib; m.second = is; m.s_best = sb; m.s_second = (is >= 0) ? ss : 0.0f;
  uint32_t nb[4];
  match_frame(c, ib, m.f);
  match_pattern(m.f, nb);
  m.dist = wv::popc64((uint64_t)(m.f[0] ^ b[0]) | ((uint64_t)(m.f[1] ^ b[1]) << 32)) +
           wv::popc64((uint64_t)(m.f[2] ^ b[2]) | ((uint64_t)(m.f[3] ^ b[3]) << 32));
  m.diff = -1;
  if (is >= 0) {
    uint32_t fs[4], ns[4];
    match_frame(c, is, fs);
    match_pattern(fs, ns);
    m.diff = wv::popc64((uint64_t)(nb[0] ^ ns[0]) | ((uint64_t)(nb[1] ^ ns[1]) << 32)) +
             wv::popc64((uint64_t)(nb[2] ^ ns[2]) | ((uint64_t)(nb[3] ^ ns[3]) << 32));
  }
  return m;
}

// decisions lane and lane + 64 of a window from its four gathered samples, into LDS
RFID_DEVICE void match_stage(float2 pa, float2 qa, float2 pb, float2 qb, float dcr, float dci, float hre, float him, float4 *r, int lane) {
  float r0, r1, q0, q1;
  quality_rq(pa, qa, dcr, dci, hre, him, r0, q0);
  quality_rq(pb, qb, dcr, dci, hre, him, r1, q1);
  float *t = reinterpret_cast<float *>(r);
  t[lane] = r0; t[lane + 64] = r1;
}

RFID_DEVICE void match_fill(rfid_match &rec, const MatFound &m, int n_cand) {
  rec.n_cand = n_cand; rec.best = m.best; rec.second = m.second;
  rec.score_best = m.s_best; rec.score_second = m.s_second; rec.sig_abs = m.sig;
  rec.dist_best = m.dist; rec.diff = m.diff;
  rec.frame[0] = m.f[0]; rec.frame[1] = m.f[1]; rec.frame[2] = m.f[2]; rec.frame[3] = m.f[3];
}

RFID_DEVICE void match_clear(rfid_match &rec) {
  rec.stream = 0; rec.seq = 0; rec.start = 0; rec.flags = 0; rec.n_cand = 0; rec.best = 0; rec.second = 0;
  rec.score_best = 0.0f; rec.score_second = 0.0f; rec.sig_abs = 0.0f; rec.dist_best = 0; rec.diff = 0;
  rec.frame[0] = rec.frame[1] = rec.frame[2] = rec.frame[3] = 0u;
}

struct MatArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  int rows;                         // ceil(wmax / 2): the row of an EPC window is seq >> 1
  int blocks;                       // ceil(rows / MAT_ROWS)
  const uint32_t *list;             // [n_list][4]: the caller's frames, or nullptr: every trace's own inventory
  int n_list;
  const rfid_tag_entry *ent;        // [n_streams][max_tags]: the inventory of the same pass (read without a list only)
  const int *ent_counts;            // [n_streams]: its entries per trace (0 when the trace overflowed)
  const int *ent_over;              // [n_streams]: 1 = the trace overflowed the inventory
  int max_tags;
  rfid_match *table;                // [n_streams][rows]
  int *nrows;                       // [n_streams]: EPC windows before the cut-off (n_windows_used / 2)
};

RFID_KERNEL(64) void match_kernel(MatArgs a) {
  RFID_SHARED float4 r[32];
  const int lane = wv::lane_id();
  const int64_t n_items = (int64_t)a.p.n_streams * a.blocks;
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int strm = (int)(it / a.blocks);
    const int r0 = (int)(it - (int64_t)strm * a.blocks) * MAT_ROWS;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, strm);
    const int nrows = nw >> 1;             // seq = 2 row + 1 < nw
    if (r0 == 0 && lane == 0) a.nrows[strm] = nrows;
    const int my_row = r0 + lane;
    const bool mine = lane < MAT_ROWS && my_row < a.rows;      // (this lane stores a row)
    const bool on = lane < MAT_ROWS && my_row < nrows;
    const int k = 2 * my_row + 1;
    rfid_match rec;
    match_clear(rec);
    if (r0 < nrows) {
      // ---- every lane its own row: window and result, all rows of the block in flight together ----
      int start = 0, index = 0, type = 0, crc_ok = 0;
      float dcr = 0.0f, dci = 0.0f, T = 0.0f, hre = 0.0f, him = 0.0f;
      int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
      if (on) {
        const rfid_window *wd = a.p.wtab + ((int64_t)strm * a.p.wmax + k);
        const rfid_decode_result *rs = a.p.res + ((int64_t)strm * a.p.wmax + k);
        start = wd->start; dcr = wd->dc_re; dci = wd->dc_im;
        type = rs->type; index = rs->index; hre = rs->h_re; him = rs->h_im; T = rs->T; crc_ok = rs->crc_ok;
        b0 = (int)rs->bits[0]; b1 = (int)rs->bits[1]; b2 = (int)rs->bits[2]; b3 = (int)rs->bits[3];
      }
      const bool ok = type == RFID_DECODE_EPC && crc_ok == 1;          // (a read, as stage_fetch has it)
      // ---- the trace's candidates ----
      MatCands c;
      int set;
      if (a.list) {
        c.f = a.list; c.stride = 4; c.n = a.n_list; set = 8;
      } else {
        const bool over = a.ent_over[strm] != 0;
        int E = over ? 0 : a.ent_counts[strm];
        if (E > a.max_tags) E = a.max_tags;
        c.f = (a.ent + (int64_t)strm * a.max_tags)->frame; c.stride = (int)(sizeof(rfid_tag_entry) / sizeof(uint32_t)); c.n = (E < 0) ? 0 : E;
        set = over ? 2 : 0;
      }
      if (c.n == 0 && !(set & 2)) set |= 4;
      if (on) { rec.stream = strm; rec.seq = k; rec.start = start; rec.flags = (ok ? 1 : 0) | set; }
      // ---- the failed rows, one after the other; the gathers of the next one are in flight meanwhile ----
      const float2 *y = a.p.y + (int64_t)strm * a.p.y_stride;
      uint64_t todo = wv::ballot(on && !ok && c.n > 0);
      float2 pa = make_float2(0.0f, 0.0f), qa = pa, pb = pa, qb = pa;
      if (todo) {
        const int nx = wv::ffs64(todo);
        epc_gather(y + wv::readlane(start, nx), wv::readlane(T, nx), (float)wv::readlane(index, nx), lane, pa, qa, pb, qb);
      }
      while (todo) {
        const int lead = wv::ffs64(todo);
        todo &= todo - 1ull;
        match_stage(pa, qa, pb, qb, wv::readlane(dcr, lead), wv::readlane(dci, lead), wv::readlane(hre, lead), wv::readlane(him, lead), r, lane);
        wv::wave_sync();
        if (todo) {
          const int nx = wv::ffs64(todo);
          epc_gather(y + wv::readlane(start, nx), wv::readlane(T, nx), (float)wv::readlane(index, nx), lane, pa, qa, pb, qb);
        }
        const uint32_t b[4] = {(uint32_t)wv::readlane(b0, lead), (uint32_t)wv::readlane(b1, lead), (uint32_t)wv::readlane(b2, lead),
                               (uint32_t)wv::readlane(b3, lead)};
        const MatFound m = match_search(r, c, b, lane);
        if (lane == lead) match_fill(rec, m, c.n);
        wv::wave_sync();   // (the next row overwrites the decision values)
      }
    }
    if (mine) a.table[(int64_t)strm * a.rows + my_row] = rec;     // (behind the cut-off: zeros)
  }
}

// ---- one caller-supplied window and list (rfid_match_window): the same gather, staging and search, one wave; gated: DC-free ----
RFID_KERNEL(64) void match_one_kernel(const float2 *gated, const rfid_decode_result *res, const uint32_t *frames, int n_frames, rfid_match *out) {
  RFID_SHARED float4 r[32];
  const int lane = wv::lane_id();
  rfid_match rec;
  match_clear(rec);
  rec.flags = (res->crc_ok & 1) | 8;
  if (!(rec.flags & 1)) {
    float2 pa, qa, pb, qb;
    epc_gather(gated, res->T, (float)res->index, lane, pa, qa, pb, qb);
    match_stage(pa, qa, pb, qb, 0.0f, 0.0f, res->h_re, res->h_im, r, lane);
    wv::wave_sync();
    MatCands c;
    c.f = frames; c.stride = 4; c.n = n_frames;
    const uint32_t b[4] = {res->bits[0], res->bits[1], res->bits[2], res->bits[3]};
    match_fill(rec, match_search(r, c, b, lane), n_frames);
  }
  if (lane == 0) *out = rec;
}

}  // namespace rfidk
