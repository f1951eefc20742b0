// rfid_slots.hpp -- the slots stage of the batched path: behind a pass, one rfid_window_moments per window before the TERMINATED
// cut-off, RN16 and EPC alike -- the five second-order sums of the window's first 240 gated samples.  The reference ACKs every
// slot (it has no empty-slot detection), so a FIXED_Q > 0 trace decodes to an RN16 / EPC window pair per slot whatever was on
// the air.  The gated samples tell: one tag's reply lies on a line in the I/Q plane (two levels along h), two tags' replies
// spread over a plane, no reply is an isotropic noise blob -- the eigenvalues of a window's 2 x 2 scatter matrix separate the
// three, and the minor eigenvalue of any EPC window is noise (rfid.batch.classify_slots, on the host: the tables are tiny).
// No counterpart in the reference: it is what a caller would otherwise work out from the matched filter's whole output.
//
// The definition (include/rfid_mi355x.h, rfid_window_moments) is in binary32, one rounding per operation, the five sums in the
// order of i from 0.0f: a record is a function of the input alone.  The kernel's shape:
//   read    a wave takes MOM_PACK = 8 windows of one trace at a time (a persistent grid over (trace, pack of rows)).  A window's
//           240 samples are contiguous: 64 lanes x float2, three full loads and one of 48 lanes, the 32 loads of the eight
//           windows in flight together.  x_i = re - dc_re and y_i = im - dc_im are formed in registers.
//   park    the (x_i, y_i) of a window go to LDS as one row of float2, rows MOM_STRIDE = 241 float2 apart: 482 words = 34 mod
//           64, so the eight rows start in the bank pairs {0,1} {34,35} {4,5} {38,39} {8,9} {42,43} {12,13} {46,47}.
//   sums    40 lanes -- one per (window, sum) -- walk a row each with one 8-byte read per step; the five walkers of a window
//           read the same address (a broadcast), the eight windows different banks.  A walker forms its own term from the pair
//           -- x, y, x x, x y or y y: a product is rounded by itself, whichever lane forms it -- and adds it in the order of i.
//           240 dependent additions for eight windows, against the 15 360 bytes the pack read.
//   store   the eight 32-byte records are put together in LDS and leave as one 256-byte row of the table, one word per lane.
// The cut-off is the other stages' (stage_windows).  Rows behind a trace's cut-off are zeroed, so the table's bytes repeat from
// pass to pass.  Single-wave workgroups, nothing shared between them, no atomics: nothing depends on the order in which they run.
// moments_of_kernel is the per-call twin: the same device function over gated samples a caller holds (dc = 0).
// Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int MOM_PACK = 8;               // windows per wave and step
constexpr int MOM_WGS_PER_CU = 8;         // most single-wave workgroups of a launch, per compute unit
constexpr int MOM_N = RFID_MOMENTS_SAMPLES;
constexpr int MOM_STRIDE = MOM_N + 1;     // float2 per parked row
constexpr int MOM_SUMS = 5;
constexpr int MOM_WORDS = (int)(sizeof(rfid_window_moments) / sizeof(int));
static_assert(sizeof(rfid_window_moments) == 32 && MOM_PACK * MOM_WORDS == 64, "one word per lane");
static_assert(MOM_PACK * MOM_SUMS <= 64, "one lane per (window, sum)");
static_assert(MOM_N == 3 * 64 + 48 && MOM_N <= RN16_WIN && MOM_N <= EPC_WIN, "three full loads and one of 48, inside either window");
static_assert((2 * MOM_STRIDE) % 64 == 34, "the eight rows start in different bank pairs");

struct MomWin {      // what a window's loads and its record need (the same in every lane)
  const float2 *src; // its first gated sample
  float dcr, dci;
  int stream, seq, flags;
};

// The records of up to eight windows (the first n_on of w; the others are read -- they name a window that may be read -- and
// their records zeroed) into rec[64], behind a wave_sync.  xy: MOM_PACK * MOM_STRIDE float2 of LDS.
RFID_DEVICE void moments_pack(float2 *xy, int *rec, const MomWin (&w)[MOM_PACK], int n_on, int lane) {
  float2 v[MOM_PACK][4];
#pragma unroll
  for (int u = 0; u < MOM_PACK; ++u) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[u][k] = w[u].src[lane + 64 * k];
    v[u][3] = (lane < MOM_N - 192) ? w[u].src[lane + 192] : make_float2(0.0f, 0.0f);
  }
#pragma unroll
  for (int u = 0; u < MOM_PACK; ++u) {
    float2 *row = xy + u * MOM_STRIDE;
#pragma unroll
    for (int k = 0; k < 3; ++k) row[lane + 64 * k] = make_float2(v[u][k].x - w[u].dcr, v[u][k].y - w[u].dci);
    if (lane < MOM_N - 192) row[lane + 192] = make_float2(v[u][3].x - w[u].dcr, v[u][3].y - w[u].dci);
    if (lane == 0) {
      const bool on = u < n_on;
      int *r = rec + u * MOM_WORDS;
      r[0] = on ? w[u].stream : 0; r[1] = on ? w[u].seq : 0; r[7] = on ? w[u].flags : 0;
    }
  }
  wv::wave_sync();
  // ---- the in-order sums: lane 5 u + c walks sum c of window u ----
  if (lane < MOM_PACK * MOM_SUMS) {
    const int u = lane / MOM_SUMS, c = lane - MOM_SUMS * u;
    const bool first_x = (c == 0) || (c == 2) || (c == 3);     // x, y, x x, x y, y y
    const float2 *t = xy + u * MOM_STRIDE;
    float acc = 0.0f;
#pragma unroll 16
    for (int i = 0; i < MOM_N; ++i) {
      const float2 p = t[i];
      const float f = first_x ? p.x : p.y;
      const float g = (c < 2) ? 1.0f : ((c == 2) ? p.x : p.y);  // (f * 1.0f is f)
      acc = acc + f * g;
    }
    rec[u * MOM_WORDS + 2 + c] = (u < n_on) ? (int)wv::f2u(acc) : 0;
  }
  wv::wave_sync();
}

struct MomArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  rfid_window_moments *table;       // [n_streams][wmax]: the row of a window is its seq
  int *nrows;                       // [n_streams]: windows before the cut-off (n_windows_used)
};

RFID_KERNEL(64) void moments_kernel(MomArgs a) {
  RFID_SHARED float2 xy[MOM_PACK * MOM_STRIDE];
  RFID_SHARED int rec[MOM_PACK * MOM_WORDS];
  const int lane = wv::lane_id();
  const int packs_per = (a.p.wmax + MOM_PACK - 1) / MOM_PACK;
  const int64_t n_items = (int64_t)a.p.n_streams * packs_per;
  int *table_w = reinterpret_cast<int *>(a.table);
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int s = (int)(it / packs_per);
    const int r0 = (int)(it - (int64_t)s * packs_per) * MOM_PACK;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, s);
    if (r0 == 0 && lane == 0) a.nrows[s] = nw;
    const int my_row = r0 + (lane >> 3);   // (the record this lane stores a word of)
    int *out = table_w + ((int64_t)s * a.p.wmax + my_row) * MOM_WORDS + (lane & 7);
    if (r0 >= nw) {                        // behind the cut-off
      if (my_row < a.p.wmax) *out = 0;
      continue;
    }
    MomWin w[MOM_PACK];
#pragma unroll
    for (int u = 0; u < MOM_PACK; ++u) {
      const int row = (r0 + u < nw) ? (r0 + u) : r0;         // (a row behind the cut-off: the pack's first, its sums unused)
      const int64_t k = (int64_t)s * a.p.wmax + row;
      const rfid_window wd = a.p.wtab[k];
      const int crc_ok = reinterpret_cast<const int *>(a.p.res + k)[10];
      w[u].src = a.p.y + (int64_t)s * a.p.y_stride + wd.start;
      w[u].dcr = wd.dc_re; w[u].dci = wd.dc_im;
      w[u].stream = s; w[u].seq = row;
      w[u].flags = (row & 1) ? (2 | (crc_ok & 1)) : 0;       // (type = seq & 1)
    }
    const int n_on = (nw - r0 < MOM_PACK) ? (nw - r0) : MOM_PACK;
    moments_pack(xy, rec, w, n_on, lane);
    if (my_row < a.p.wmax) *out = rec[lane];
    wv::wave_sync();   // (the next pack overwrites both areas)
  }
}

// ---- the per-call twin: n_windows x 240 gated, DC-free samples a caller holds -> one record each -------------------------
RFID_KERNEL(64) void moments_of_kernel(const float2 *gated, int n_windows, rfid_window_moments *out) {
  RFID_SHARED float2 xy[MOM_PACK * MOM_STRIDE];
  RFID_SHARED int rec[MOM_PACK * MOM_WORDS];
  const int lane = wv::lane_id();
  const int packs = (n_windows + MOM_PACK - 1) / MOM_PACK;
  int *out_w = reinterpret_cast<int *>(out);
  for (int it = (int)blockIdx.x; it < packs; it += (int)gridDim.x) {
    const int r0 = it * MOM_PACK;
    MomWin w[MOM_PACK];
#pragma unroll
    for (int u = 0; u < MOM_PACK; ++u) {
      const int row = (r0 + u < n_windows) ? (r0 + u) : r0;
      w[u].src = gated + (int64_t)row * MOM_N;
      w[u].dcr = 0.0f; w[u].dci = 0.0f;
      w[u].stream = 0; w[u].seq = row; w[u].flags = 0;
    }
    const int n_on = (n_windows - r0 < MOM_PACK) ? (n_windows - r0) : MOM_PACK;
    moments_pack(xy, rec, w, n_on, lane);
    const int my_row = r0 + (lane >> 3);
    if (my_row < n_windows) out_w[(int64_t)my_row * MOM_WORDS + (lane & 7)] = rec[lane];
    wv::wave_sync();
  }
}

}  // namespace rfidk
