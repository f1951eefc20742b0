// rfid_stage.hpp -- what the stages behind a batch pass decide in the same way, written once.  Every stage header includes
// this file and, beside it, only the stage headers whose symbols it uses (the tracks: the inventory's table walk).
//   stage_windows / stage_fetch   which windows of a trace count in a pass, how a result record is read and which records are
//                                 reads (all thirteen stages / inventory and tracks);
//   scan_share / scan_partials    the one-workgroup offsets scan (inventory, tracks; the repair stage takes the shares);
//   StagePass                     what a pass left, as the eleven window-table stages see it -- quality, repair, slots, commands,
//                                 fine, retune, collisions, lengths, diversity, match, stack: each fills one [trace][row] table (the diversity stage: [group][row]) of fixed-size records with a persistent grid of single-wave
//                                 workgroups, stage_windows gives the cut-off, rows behind it are zeroed, nrows[s] is written by
//                                 the first pack.  How a table kernel loads, parks, sums and stores is its own (its header says why);
//   epc_clamp / epc_gather        the decoder's half-bit gather of an EPC window (quality, repair, fine, diversity, match, stack);
//   table_gather_kernel           the table's records of the CRC-verified reads, aligned with the tracks (quality, fine).
// Only primitives both device environments offer.
#pragma once
#include "rfid_kernels.hpp"

namespace rfidk {

// the windows of trace s that count in this pass: those the gate opened, before the TERMINATED cut-off
RFID_DEVICE int stage_windows(const int *wcount, const rfid_stream_stats *stats, int wmax, int s) {
  int nw = wcount[s];
  const int used = stats[s].n_windows_used;
  if (used < nw) nw = used;
  if (nw > wmax) nw = wmax;
  return (nw < 0) ? 0 : nw;
}

// one result record as the inventory and the tracks kernels read it
struct StageRead {
  uint32_t f[4];
  int h_re, h_im, T, index;   // (bit patterns)
  bool on;                    // an EPC window with a verified CRC
};

RFID_DEVICE StageRead stage_fetch(const rfid_decode_result *rs, int k, int k_end) {
  StageRead q;
  q.f[0] = q.f[1] = q.f[2] = q.f[3] = 0u; q.h_re = q.h_im = q.T = q.index = 0; q.on = false;
  if (k < k_end) {
    // the whole 48-byte record in three 16-byte loads, none of them waiting for another (rows are 16-byte aligned)
    static_assert(sizeof(rfid_decode_result) == 48, "rfid_decode_result is read as 12 words");
    const int *p = reinterpret_cast<const int *>(rs + k);
    int w[12];
    wv::load4_i32(p, w[0], w[1], w[2], w[3]);        // type, index, h_re, h_im
    wv::load4_i32(p + 4, w[4], w[5], w[6], w[7]);    // T, bits[0..2]
    wv::load4_i32(p + 8, w[8], w[9], w[10], w[11]);  // bits[3], n_bits, crc_ok, tag_id
    if (w[0] == RFID_DECODE_EPC && w[10] == 1) {
      q.on = true;
      q.f[0] = (uint32_t)w[5]; q.f[1] = (uint32_t)w[6]; q.f[2] = (uint32_t)w[7]; q.f[3] = (uint32_t)w[8];
      q.index = w[1]; q.h_re = w[2]; q.h_im = w[3]; q.T = w[4];
    }
  }
  return q;
}

// The one-workgroup offsets scan over per-trace amounts (inventory_offsets_kernel, tracks_offsets_kernel): every thread
// sums the amounts of a contiguous share of the traces, thread 0 scans the partial sums serially (INV_SCAN_THREADS at
// most), every thread then walks its share again from the base it is handed.
constexpr int INV_SCAN_THREADS = 1024;

struct ScanShare { int b0, b1; };     // this thread's traces: [b0, b1)
RFID_DEVICE ScanShare scan_share(int n_streams, int tid, int nthr) {
  const int per = (n_streams + nthr - 1) / nthr;
  ScanShare sh;
  sh.b0 = tid * per;
  sh.b1 = (sh.b0 + per < n_streams) ? (sh.b0 + per) : n_streams;
  return sh;
}

// `sum`: what this thread's share holds.  -> what the shares of the threads before it hold; `total` (thread 0 only):
// what all hold.  Two workgroup barriers: what the threads wrote to LDS before the call is visible behind it.
RFID_DEVICE int scan_partials(int *part, int tid, int nthr, int sum, int &total) {
  part[tid] = sum;
  wv::block_sync();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < nthr; ++t) { const int v = part[t]; part[t] = run; run += v; }
    total = run;
  }
  wv::block_sync();
  return part[tid];
}

// ---- the window-table stages -----------------------------------------------------------------------------------------
// What a pass left: the FIRST member of QualArgs, RepArgs, MomArgs, CmdArgs, FineArgs, RetArgs, ColArgs, LenArgs, DivArgs, MatArgs and StkArgs, filled by the host's table_begin.
// (InvArgs and TrkArgs carry no y and another order: they stay their own.)
struct StagePass {
  const float2 *y;                  // the matched filter's output of the pass
  int64_t y_stride;
  const rfid_window *wtab;          // [n_streams][wmax]
  const rfid_decode_result *res;    // [n_streams][wmax]
  const int *wcount;                // [n_streams]
  const rfid_stream_stats *stats;   // [n_streams]: n_windows_used of the same pass
  int wmax, n_streams;
};

// The stages that read behind a window (retune, lengths; the diversity stage inside a window) never read behind the trace's own length.
// the matched-filter outputs trace s holds (as gate_extent has it); lens: raw samples per trace, or nullptr: n_dec for all
RFID_DEVICE int stage_extent(const int64_t *lens, int64_t n_dec, int s) {
  int64_t n64 = n_dec;
  if (lens) {
    int64_t r = lens[s];
    if (r < 0) r = 0;
    n64 = r / DECIM;
    if (n64 > n_dec) n64 = n_dec;
  }
  return (int)n64;
}
// the last own sample of a span of `span` samples that starts at `start` in a trace of n_dec outputs (-1: none)
RFID_DEVICE int stage_span_last(int n_dec, int start, int span) {
  if (start < 0 || start >= n_dec) return -1;
  const int last = n_dec - 1 - start;
  return (last > span - 1) ? (span - 1) : last;
}

RFID_DEVICE int epc_clamp(int i) { return (i < 0) ? 0 : ((i > EPC_WIN - 1) ? (EPC_WIN - 1) : i); }

// The decoder's own gather (tag_decoder_impl.cc:171-190) of decisions j = lane and lane + 64 of the EPC window at src: the two
// half-bit samples of each (pa, qa / pb, qb), indices held inside the window (not reached: they end at 1356).  One copy: the
// index expressions round as the decoder's do, and every stage that looks at a decision must look at the same two samples.
RFID_DEVICE void epc_gather(const float2 *src, float T, float fidx, int lane, float2 &pa, float2 &qa, float2 &pb, float2 &qb) {
  const float T2 = 2.0f * T;
  const int j0 = lane, j1 = lane + 64;
  pa = src[epc_clamp(epc_index_a(j0, T2, fidx))];
  qa = src[epc_clamp(epc_index_b(j0, T, fidx))];
  pb = src[epc_clamp(epc_index_a(j1, T2, fidx))];
  qb = src[epc_clamp(epc_index_b(j1, T, fidx))];
}

// ---- the records of the CRC-verified reads, aligned with the tracks: out[i] belongs to reads[i] --------------------------
struct TableGatherArgs {
  const rfid_tag_read *reads;       // the tracks of the same pass
  const int *head;                  // [0] reads in all
  int64_t cap;
  const int *table;                 // [n_streams][rows] records of WORDS words (an EPC window's row is seq >> 1)
  int n_streams, rows;
  int *out;                         // [cap] records
};

constexpr int TABLE_GATHER_THREADS = 256;

template <int WORDS>
RFID_KERNEL(TABLE_GATHER_THREADS) void table_gather_kernel(TableGatherArgs a) {
  int64_t total = a.head[0];
  if (total > a.cap) total = a.cap;
  const int64_t n = total * WORDS, step = (int64_t)gridDim.x * TABLE_GATHER_THREADS;
  for (int64_t t = (int64_t)blockIdx.x * TABLE_GATHER_THREADS + (int64_t)threadIdx.x; t < n; t += step) {   // a word per thread
    const int64_t i = t / WORDS;
    const int word = (int)(t - i * WORDS);
    const int s = a.reads[i].stream, row = a.reads[i].seq >> 1;
    int v = 0;
    if (s >= 0 && s < a.n_streams && row >= 0 && row < a.rows) v = a.table[((int64_t)s * a.rows + row) * WORDS + word];
    a.out[t] = v;
  }
}

}  // namespace rfidk
