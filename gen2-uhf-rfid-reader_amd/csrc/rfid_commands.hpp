// rfid_commands.hpp -- the commands stage of the batched path: behind a pass, one rfid_command per window before the TERMINATED
// cut-off, RN16 and EPC alike -- the reader's own PIE command that opened the window.  Every window the gate opens was opened by
// a command on the same trace (a Query or QueryRep before an RN16 window, an ACK before an EPC window); the gate only counts its
// pulses and discards it.  It sits in the RFID_CMD_SPAN = 704 samples of the matched filter's output before the window's start,
// at full carrier depth, so it decodes where tags do not: which command, which Q, which RN16 the reader ACKed -- and whether that
// is the RN16 decoded in the window before, a reader-side ground truth that needs no CRC.
// No counterpart in the reference (its reader knows what it sent).
//
// The definition (include/rfid_mi355x.h, rfid_command) is integer apart from one binary32 comparison per sample: a record is a
// function of the input alone.  One wave takes one window at a time, up to CMD_ROWS = 16 consecutive rows of one trace per step
// (a persistent grid over (trace, block of rows); the host makes the blocks as small as the launch has waves for: a small batch
// gets a wave per window); the kernel is wave-level bit work, no float sums:
//   block    lanes 0..15 fetch the window records of the block's rows (and the RN16 result in front of an EPC window) at once: one
//            round trip for sixteen windows; a window's start, dc and RN16 are broadcast from its lane.  A block wholly behind
//            the cut-off fetches nothing and stores zeros.
//   read     the span's 704 samples are contiguous: 64 lanes x float2, eleven loads in flight together -- those of the NEXT window
//            are issued before this one is worked on.  A position before the trace's start is HIGH and its ADDRESS is clamped
//            into the trace's own row as well as its value: no read is ever formed below the row (a trace at batch index >= 1
//            would read its neighbour's tail).
//   low      low[p] = (re re + im im) < 0.25 |dc|^2, eleven ballots: the span as eleven 64-bit words, the same in every lane.
//   edges    rising edges by shift-with-carry across the words: edge = ~low & (low << 1 | carry of the word before).
//   rank     an edge's rank from the END is the popcount of the edge bits above it; the last min(n_edges, 64) edges -- rank < 64
//            -- write their position to LDS slot n - 1 - rank, so that lane j holds e_j behind a wave_sync.
//   suffix   distances from the neighbour slot; one ballot of d > RFID_CMD_GAP, its highest set bit (popcount of the smeared
//            mask) is where the command begins.
//   bits     rtcal broadcast from its lane; one ballot of 2 d > rtcal gives the data bits, aligned by a shift.
//   record   classification, CRC-5 and the comparison with the RN16 of window seq - 1 are uniform work; the sixteen 48-byte
//            records are put together in LDS and leave as 768 contiguous bytes of the table, one word per lane and store.
// The cut-off is the other stages' (stage_windows).  Rows behind a trace's cut-off are zeroed, so the table's bytes repeat from
// pass to pass.  Single-wave workgroups, nothing shared between them, no atomics: nothing depends on the order in which they run.
// commands_of_kernel is the per-call twin: the same device functions over spans a caller holds.
// Only primitives both device environments offer.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

constexpr int CMD_WGS_PER_CU = 20;        // most single-wave workgroups of a launch, per compute unit (a step is a chain of round
                                          // trips and 1 KB of LDS: as many waves as a compute unit held when this was chosen -- the
                                          // compiler then gave the kernel 87 VGPRs, five waves per SIMD.  Nothing pins that figure:
                                          // `make resource-usage` shows the current one; a larger grid only queues, a smaller one idles)
constexpr int CMD_ROWS = 16;              // rows per wave and step
constexpr int CMD_SPAN = RFID_CMD_SPAN;
constexpr int CMD_LOADS = CMD_SPAN / 64;  // float2 loads per lane
constexpr int CMD_WORDS = (int)(sizeof(rfid_command) / sizeof(int));
constexpr int CMD_BLOCK_WORDS = CMD_ROWS * CMD_WORDS;
static_assert(sizeof(rfid_command) == 48 && CMD_BLOCK_WORDS == 3 * 64, "a block's records: three words per lane");
static_assert(CMD_SPAN == 64 * CMD_LOADS, "whole ballots");
static_assert(RFID_CMD_MAX_EDGES == 64 && CMD_ROWS <= 64, "one kept edge per lane, one row per lane");

// Gen2 CRC-5 (x^5 + x^3 + 1, preset 01001, MSB first) over the 17 bits sent first: equal to the five sent behind them?
RFID_DEVICE bool cmd_crc5_holds(uint32_t bits) {
  uint32_t reg = 0x09u;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
    const uint32_t msb = (reg >> 4) & 1u;
    reg = (reg << 1) & 0x1Fu;
    if (msb ^ ((bits >> k) & 1u)) reg ^= 0x09u;
  }
  uint32_t sent = 0u;   // (bit 17 is the register's bit 4)
#pragma unroll
  for (int i = 0; i < 5; ++i) sent |= ((bits >> (17 + i)) & 1u) << (4 - i);
  return sent == reg;
}

// The span in front of a window: row = the first sample of the trace's own row, row_len samples long; a = the window's start in it
// (span position p is row[a - 704 + p]).  Address AND value are clamped for positions before the row (cmd_record looks at a again).
RFID_DEVICE void cmd_load(float2 (&v)[CMD_LOADS], const float2 *row, int64_t row_len, int a, int lane) {
#pragma unroll
  for (int k = 0; k < CMD_LOADS; ++k) {
    int64_t i = (int64_t)a - CMD_SPAN + 64 * k + lane;
    i = (i < 0) ? 0 : i;
    i = (i >= row_len) ? (row_len - 1) : i;
    v[k] = row[i];
  }
}

// The record of one window into rec[CMD_WORDS] (no wave_sync behind it).  v: its span (cmd_load with the same a); (dr, di): its
// dc; rn16_before: the low 16 decoded bits of window seq - 1 (used when check_echo).  edges: 64 ints of LDS.
RFID_DEVICE void cmd_record(int *edges, int *rec, const float2 (&v)[CMD_LOADS], int a, float dr, float di, int stream, int seq,
                            int type_flag, bool check_echo, uint32_t rn16_before, int lane) {
  const int first = a - CMD_SPAN;
  const float thr = 0.25f * (dr * dr + di * di);
  // ---- low, edges ----
  uint64_t edge[CMD_LOADS];
  uint64_t carry = 0;   // (position 0 has no predecessor: no edge there)
  int n_edges = 0;
#pragma unroll
  for (int k = 0; k < CMD_LOADS; ++k) {
    const bool clipped = first + 64 * k + lane < 0;
    const float mag = v[k].x * v[k].x + v[k].y * v[k].y;
    const uint64_t low = wv::ballot(!clipped && mag < thr);
    edge[k] = ~low & ((low << 1) | carry);
    carry = low >> 63;
    n_edges += wv::popc64(edge[k]);
  }
  const int n = (n_edges < RFID_CMD_MAX_EDGES) ? n_edges : RFID_CMD_MAX_EDGES;
  // ---- rank from the end; the kept edges to LDS, e_j in slot j ----
  wv::wave_sync();      // (the window before has read its edges)
  const uint64_t above = (lane == 63) ? 0ull : (~0ull << (lane + 1));   // the bits of a word above this lane's
  int behind = 0;                                                      // edges in the words behind word k
#pragma unroll
  for (int k = CMD_LOADS - 1; k >= 0; --k) {
    const int rank = behind + wv::popc64(edge[k] & above);
    if (((edge[k] >> lane) & 1ull) && rank < n) edges[n - 1 - rank] = 64 * k + lane;
    behind += wv::popc64(edge[k]);
  }
  wv::wave_sync();
  // ---- the command: the longest suffix without a distance above the gap ----
  const int e = (lane < n) ? edges[lane] : 0;
  const int d = (lane >= 1 && lane < n) ? (e - edges[lane - 1]) : 0;
  uint64_t brk = wv::ballot(d > RFID_CMD_GAP);
  brk |= brk >> 1; brk |= brk >> 2; brk |= brk >> 4; brk |= brk >> 8; brk |= brk >> 16; brk |= brk >> 32;
  const int c0 = brk ? (wv::popc64(brk) - 1) : 0;   // (the highest set bit: the edge behind the last long distance)
  const int m = n - c0;
  const int end = (m > 0) ? wv::readlane(e, (n - 1) & 63) : 0;
  const int d1 = wv::readlane(d, (c0 + 1) & 63), d2 = wv::readlane(d, (c0 + 2) & 63), d3 = wv::readlane(d, (c0 + 3) & 63);
  const int d0 = (m >= 2) ? d1 : 0;
  const int rtcal = (m >= 3) ? d2 : 0;
  const int trcal = (m >= 4 && d3 > rtcal) ? d3 : 0;
  const int k0 = c0 + (trcal ? 4 : 3);              // the lane of the first data symbol
  const uint64_t ones = wv::ballot(lane < n && 2 * d > rtcal);
  const int n_bits = (m >= 3) ? (n - k0) : 0;
  const uint32_t bits = (n_bits > 0) ? (uint32_t)(ones >> k0) : 0u;   // (n_bits > 0: k0 < n <= 64)
  // ---- classification: uniform ----
  int cmd = RFID_CMD_NONE;
  int flags = type_flag | ((n_edges > RFID_CMD_MAX_EDGES) ? 8 : 0) | ((first < 0) ? 16 : 0);
  if (m >= 3) {
    cmd = RFID_CMD_UNKNOWN;
    if (trcal > 0) {
      if (n_bits == 22 && (bits & 0xFu) == 0x1u) cmd = RFID_CMD_QUERY;
    } else if (n_bits == 4 && (bits & 0x3u) == 0x0u) cmd = RFID_CMD_QUERY_REP;
    else if (n_bits == 18 && (bits & 0x3u) == 0x2u) cmd = RFID_CMD_ACK;
    else if (n_bits == 8 && (bits & 0xFFu) == 0x03u) cmd = RFID_CMD_NAK;
    else if (n_bits == 9 && (bits & 0xFu) == 0x9u) cmd = RFID_CMD_QUERY_ADJUST;
    if (cmd == RFID_CMD_QUERY && cmd_crc5_holds(bits)) flags |= 2;
    if (cmd == RFID_CMD_ACK && check_echo && ((bits >> 2) & 0xFFFFu) == (rn16_before & 0xFFFFu)) flags |= 4;
    if (2 * d0 > rtcal) flags |= 32;
  }
  if (lane == 0) {
    rec[0] = stream; rec[1] = seq; rec[2] = cmd; rec[3] = n_edges; rec[4] = m; rec[5] = end;
    rec[6] = d0; rec[7] = rtcal; rec[8] = trcal; rec[9] = n_bits; rec[10] = (int)bits; rec[11] = flags;
  }
}

// One block of up to CMD_ROWS windows: the records of the first n_on into rec[CMD_BLOCK_WORDS], zeros behind them, behind a
// wave_sync.  Lane u < n_on holds window u's start, dc and the RN16 word in front of it (a_l, dr_l, di_l, rn_l).  BATCH: every
// window lies in the one row `base` (row_len samples), seq = seq0 + u, type and echo check by seq's parity; else window u has the
// row base + 704 u of its own (a_l = 704), no type, no echo check.
template <bool BATCH>
RFID_DEVICE void cmd_block(int *edges, int *rec, const float2 *base, int64_t row_len, int a_l, float dr_l, float di_l, int rn_l,
                           int stream, int seq0, int n_on, int lane) {
  float2 v[CMD_LOADS], nx[CMD_LOADS];
  int a = wv::readlane(a_l, 0);
  cmd_load(v, base, row_len, a, lane);
#pragma unroll
  for (int k = lane; k < CMD_BLOCK_WORDS; k += 64)
    if (k >= n_on * CMD_WORDS) rec[k] = 0;
  for (int u = 0; u < n_on; ++u) {
    int a_next = 0;
    if (u + 1 < n_on) {      // (the next window's loads, in flight while this one is worked on)
      a_next = wv::readlane(a_l, u + 1);
      cmd_load(nx, BATCH ? base : base + (int64_t)(u + 1) * CMD_SPAN, row_len, a_next, lane);
    }
    const int seq = seq0 + u;
    cmd_record(edges, rec + u * CMD_WORDS, v, a, wv::readlane(dr_l, u), wv::readlane(di_l, u), stream, seq, BATCH ? (seq & 1) : 0,
               BATCH && (seq & 1), (uint32_t)wv::readlane(rn_l, u), lane);
    if (u + 1 < n_on) {
#pragma unroll
      for (int k = 0; k < CMD_LOADS; ++k) v[k] = nx[k];
      a = a_next;
    }
  }
  wv::wave_sync();
}

struct CmdArgs {
  StagePass p;                      // what the pass left (rfid_stage.hpp)
  rfid_command *table;              // [n_streams][wmax]: the row of a window is its seq
  int *nrows;                       // [n_streams]: windows before the cut-off (n_windows_used)
  int rows_per;                     // rows per wave and step, 1..CMD_ROWS (the host's choice: 1 while the launch has a wave per row)
};

RFID_KERNEL(64) void commands_kernel(CmdArgs a) {
  RFID_SHARED int edges[RFID_CMD_MAX_EDGES];
  RFID_SHARED int rec[CMD_BLOCK_WORDS];
  const int lane = wv::lane_id();
  const int R = a.rows_per;
  const int blocks_per = (a.p.wmax + R - 1) / R;
  const int64_t n_items = (int64_t)a.p.n_streams * blocks_per;
  int *table_w = reinterpret_cast<int *>(a.table);
  for (int64_t it = (int64_t)blockIdx.x; it < n_items; it += (int64_t)gridDim.x) {
    const int s = (int)(it / blocks_per);
    const int r0 = (int)(it - (int64_t)s * blocks_per) * R;
    const int nw = stage_windows(a.p.wcount, a.p.stats, a.p.wmax, s);
    if (r0 == 0 && lane == 0) a.nrows[s] = nw;
    const int rows = (a.p.wmax - r0 < R) ? (a.p.wmax - r0) : R;   // (the table's rows of this block)
    int *out = table_w + ((int64_t)s * a.p.wmax + r0) * CMD_WORDS;
    if (r0 >= nw) {                        // behind the cut-off
#pragma unroll
      for (int k = lane; k < CMD_BLOCK_WORDS; k += 64)
        if (k < rows * CMD_WORDS) out[k] = 0;
      continue;
    }
    const int n_on = (nw - r0 < R) ? (nw - r0) : R;
    int a_l = 0, rn_l = 0;
    float dr_l = 0.0f, di_l = 0.0f;
    if (lane < n_on) {
      const int64_t k = (int64_t)s * a.p.wmax + r0 + lane;
      const rfid_window wd = a.p.wtab[k];
      a_l = wd.start; dr_l = wd.dc_re; di_l = wd.dc_im;
      // the RN16 the window before decoded (results are read as words, as stage_fetch reads them: bits[0] is word 5)
      if ((r0 + lane) & 1) rn_l = reinterpret_cast<const int *>(a.p.res + (k - 1))[5];
    }
    cmd_block<true>(edges, rec, a.p.y + (int64_t)s * a.p.y_stride, a.p.y_stride, a_l, dr_l, di_l, rn_l, s, r0, n_on, lane);
#pragma unroll
    for (int k = lane; k < CMD_BLOCK_WORDS; k += 64)
      if (k < rows * CMD_WORDS) out[k] = rec[k];
    wv::wave_sync();   // (the next block overwrites rec)
  }
}

// ---- the per-call twin: n spans of 704 samples a caller holds, the dc of each -> one record each ---------------------------
RFID_KERNEL(64) void commands_of_kernel(const float2 *spans, const float2 *levels, int n, rfid_command *out) {
  RFID_SHARED int edges[RFID_CMD_MAX_EDGES];
  RFID_SHARED int rec[CMD_BLOCK_WORDS];
  const int lane = wv::lane_id();
  const int blocks = (n + CMD_ROWS - 1) / CMD_ROWS;
  int *out_w = reinterpret_cast<int *>(out);
  for (int it = (int)blockIdx.x; it < blocks; it += (int)gridDim.x) {
    const int r0 = it * CMD_ROWS;
    const int n_on = (n - r0 < CMD_ROWS) ? (n - r0) : CMD_ROWS;
    float2 lv = make_float2(0.0f, 0.0f);
    if (lane < n_on) lv = levels[r0 + lane];
    cmd_block<false>(edges, rec, spans + (int64_t)r0 * CMD_SPAN, CMD_SPAN, CMD_SPAN, lv.x, lv.y, 0, 0, r0, n_on, lane);
#pragma unroll
    for (int k = lane; k < CMD_BLOCK_WORDS; k += 64)
      if (k < n_on * CMD_WORDS) out_w[(int64_t)r0 * CMD_WORDS + k] = rec[k];
    wv::wave_sync();
  }
}

}  // namespace rfidk
