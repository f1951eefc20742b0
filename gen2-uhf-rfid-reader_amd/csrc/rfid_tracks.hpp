// rfid_tracks.hpp -- the tracks stage of the batched path: behind the inventory of a pass, every CRC-verified EPC read
// before the TERMINATED cut-off as one rfid_tag_read (when it happened, and the h_est / T / index the decoder formed
// for it), grouped by tag and in time order inside a tag: ordered by (stream, entry, seq).  No counterpart in the
// reference: it is what a caller would otherwise group on the host from every window and result of a pass.
//
// A read's place is  base(stream) + reads of the trace's earlier entries + earlier reads of the same frame  -- a
// function of the input alone.  A stable counting scatter finds it in linear time, one workgroup per trace:
//   table   the trace's entries (<= 512 distinct frames, listed by the inventory in the order of their first reads)
//           are put into a hash table in LDS, the ENTRY INDEX as the owner of a slot.  Probe sequence, hash and the
//           walk that finds a frame are the inventory's (inv_hash, inv_walk); the round scheme is of its kind and needs no
//           compare-and-swap either: in a round every entry not
//           yet placed walks its probes over settled[] (the owners as they stood when the round began) to the first
//           empty slot and asks for it with atomic_min; behind a barrier the winner settles with its key, the others
//           move one probe on.  The lowest index among those that ask always wins: at most as many rounds as entries,
//           two with the default table, and the table is the same whichever wave got where first.
//   pass 1  (sixteen waves only) every wave owns a contiguous range of the windows and counts its reads per entry:
//           cur[entry][wave].  One wave: the entry's own read count is the number.
//   prefix  over the waves of an entry, then over the entries: cur[entry][wave] becomes the place of the first read of
//           that entry in that wave's range.
//   pass 2  every wave walks its range in batches of 64 windows, in order.  Inside a batch the lanes that hold the same
//           entry are found with ballot; a lane's rank is the number of lower lanes among them, the lowest of them
//           moves the cursor on by their number (an LDS atomic whose old value readlane hands to the others).
// Which windows count (stage_windows) and how a result record is read (stage_fetch) are every stage's (rfid_stage.hpp).
// Only primitives both device environments offer, workgroup barriers only, nothing shared between workgroups.
#pragma once
#include "rfid_inventory.hpp"

namespace rfidk {

// ---- bases: the reads of the traces before each trace (one workgroup; scan_share / scan_partials as inventory_offsets_kernel) --------
struct TrkScanArgs {
  const rfid_tag_entry *ent;    // [n_streams][max_tags]: the inventory's rows
  const int *counts;            // [n_streams]: entries per trace (0 when the trace overflowed)
  const int *inv_head;          // [0] entries in all
  int n_streams, max_tags;
  int *base;                    // [n_streams]: reads of the traces before this one
  int *head;                    // [0] reads in all
  int64_t *offsets;             // [entries in all + 1]: the last one is written here, the others by tracks_kernel
};

RFID_KERNEL(INV_SCAN_THREADS) void tracks_offsets_kernel(TrkScanArgs a) {
  RFID_SHARED int part[INV_SCAN_THREADS];
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const ScanShare sh = scan_share(a.n_streams, tid, nthr);
  int sum = 0;
  for (int b = sh.b0; b < sh.b1; ++b) {
    const rfid_tag_entry *e = a.ent + (int64_t)b * a.max_tags;
    const int n = a.counts[b];
    for (int i = 0; i < n; ++i) sum += e[i].reads;
  }
  int total = 0;
  int run = scan_partials(part, tid, nthr, sum, total);
  if (tid == 0) {
    a.head[0] = total;
    a.offsets[a.inv_head[0]] = total;
  }
  for (int b = sh.b0; b < sh.b1; ++b) {
    a.base[b] = run;
    const rfid_tag_entry *e = a.ent + (int64_t)b * a.max_tags;
    const int n = a.counts[b];
    for (int i = 0; i < n; ++i) run += e[i].reads;
  }
}

// ---- the scatter ------------------------------------------------------------------------------------------------------
struct TrkArgs {
  const rfid_decode_result *res;    // [n_streams][wmax]
  const rfid_window *wtab;          // [n_streams][wmax]
  const int *wcount;                // [n_streams]
  const rfid_stream_stats *stats;   // [n_streams]: n_windows_used of the same pass
  int wmax, n_streams;
  const rfid_tag_entry *ent;        // [n_streams][max_tags]: the inventory of the same pass
  const int *counts;                // [n_streams]: its entries per trace (0 when the trace overflowed)
  const int *ent_off;               // [n_streams]: entries of the traces before this one (the packed list's offsets)
  int max_tags;
  int slots;                        // power of two, 2 .. SLOTS of the instantiation, >= the entries of any trace
  const int *base;                  // [n_streams]: tracks_offsets_kernel
  rfid_tag_read *out;               // [cap]
  int64_t cap;
  int64_t *offsets;                 // [entries in all + 1], aligned with the packed entries
};

// the entry that holds this frame: all S probes of inv_walk, then the slot's owner.  -1 when none does (not reached
// behind an inventory of the same results)
RFID_DEVICE int trk_find(const uint32_t (&f)[4], const int *settled, const uint32_t *key, int S) {
  int empty_slot = 0;
  const int slot = inv_walk(f, settled, key, S - 1, S - 1, empty_slot);
  return (slot >= 0) ? settled[slot] : -1;
}

// One workgroup per trace: WAVES = 1, or 16 when a trace can hold thousands of windows (the host picks, as for
// inventory_kernel).  ENT: the most entries a trace can have (max_tags <= ENT).
template <int SLOTS, int ENT, int WAVES>
RFID_KERNEL(64 * WAVES) void tracks_kernel(TrkArgs a) {
  RFID_SHARED int owner[SLOTS];
  RFID_SHARED int settled[SLOTS];
  RFID_SHARED uint32_t key[4 * SLOTS];
  RFID_SHARED int cur[ENT * WAVES];   // pass 1: reads of (entry, wave); behind the prefix: where its next read goes
  RFID_SHARED int aux[ENT];           // table: the probe an entry stands at (-1: placed); then: reads before the entry
  RFID_SHARED int sh_again;
  constexpr int nthr = 64 * WAVES;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = (int)blockIdx.x;
  if (s >= a.n_streams) return;
  int E = a.counts[s];
  if (E > ENT) E = ENT;               // (not reached: the host picks ENT >= max_tags)
  if (E <= 0) return;                 // no verified read, or a trace that overflowed the inventory: lists nothing
  const int S = a.slots, mask = S - 1;
  const rfid_tag_entry *ent = a.ent + (int64_t)s * a.max_tags;
  for (int i = tid; i < S; i += nthr) { owner[i] = INV_EMPTY; settled[i] = INV_EMPTY; }
  for (int e = tid; e < E; e += nthr) aux[e] = 0;
  for (int i = tid; i < E * WAVES; i += nthr) cur[i] = 0;
  if (tid == 0) sh_again = 0;
  wv::block_sync();
  // ---- the table ----
  for (;;) {
    for (int e = tid; e < E; e += nthr) {
      int i = aux[e];
      if (i < 0) continue;
      const uint32_t f[4] = {ent[e].frame[0], ent[e].frame[1], ent[e].frame[2], ent[e].frame[3]};
      int h0, step;
      inv_hash(f, mask, h0, step);
      while (i < S && settled[(h0 + i * step) & mask] != INV_EMPTY) ++i;
      aux[e] = i;
      if (i < S) wv::atomic_min(&owner[(h0 + i * step) & mask], e);
      sh_again = 1;     // (every writer stores the same value)
    }
    wv::block_sync();
    const bool again = sh_again != 0;
    if (!again) break;
    wv::block_sync();                       // (all have read sh_again)
    for (int e = tid; e < E; e += nthr) {
      const int i = aux[e];
      if (i < 0) continue;
      if (i >= S) { aux[e] = -1; continue; }     // (not reached: no more entries than slots)
      const uint32_t f[4] = {ent[e].frame[0], ent[e].frame[1], ent[e].frame[2], ent[e].frame[3]};
      int h0, step;
      inv_hash(f, mask, h0, step);
      const int slot = (h0 + i * step) & mask;
      if (owner[slot] == e) {
        settled[slot] = e;
        key[4 * slot + 0] = f[0]; key[4 * slot + 1] = f[1]; key[4 * slot + 2] = f[2]; key[4 * slot + 3] = f[3];
        aux[e] = -1;
      } else {
        aux[e] = i + 1;
      }
    }
    if (tid == 0) sh_again = 0;
    wv::block_sync();
  }
  const int nw = stage_windows(a.wcount, a.stats, a.wmax, s);
  const rfid_decode_result *rs = a.res + (int64_t)s * a.wmax;
  const rfid_window *wt = a.wtab + (int64_t)s * a.wmax;
  // this wave's windows: a contiguous range, a multiple of 64 long
  const int per = (((nw + WAVES - 1) / WAVES) + 63) & ~63;
  const int k0 = (wave * per < nw) ? (wave * per) : nw;
  const int k1 = (k0 + per < nw) ? (k0 + per) : nw;
  // ---- pass 1 ----
  if (WAVES > 1) {
    for (int base = k0; base < k1; base += 64 * INV_UNROLL) {
      StageRead q[INV_UNROLL];
#pragma unroll
      for (int u = 0; u < INV_UNROLL; ++u) q[u] = stage_fetch(rs, base + u * 64 + lane, k1);
#pragma unroll
      for (int u = 0; u < INV_UNROLL; ++u) {
        if (!q[u].on) continue;
        const int e = trk_find(q[u].f, settled, key, S);
        if (e >= 0) wv::atomic_add(&cur[e * WAVES + wave], 1);
      }
    }
    wv::block_sync();
  }
  // ---- prefix: over the waves of an entry, over the entries ----
  for (int e = tid; e < E; e += nthr) {
    if (WAVES > 1) {
      int run = 0;
      for (int w = 0; w < WAVES; ++w) { const int v = cur[e * WAVES + w]; cur[e * WAVES + w] = run; run += v; }
      aux[e] = run;
    } else {
      aux[e] = ent[e].reads;
    }
  }
  wv::block_sync();
  if (tid == 0) {
    int run = a.base[s];
    for (int e = 0; e < E; ++e) { const int v = aux[e]; aux[e] = run; run += v; }
  }
  wv::block_sync();
  {
    int64_t *off = a.offsets + a.ent_off[s];
    for (int e = tid; e < E; e += nthr) {
      const int first = aux[e];
      off[e] = first;
      for (int w = 0; w < WAVES; ++w) cur[e * WAVES + w] += first;
    }
  }
  wv::block_sync();
  // ---- pass 2 ----
  for (int base = k0; base < k1; base += 64 * INV_UNROLL) {
    StageRead q[INV_UNROLL];
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) q[u] = stage_fetch(rs, base + u * 64 + lane, k1);
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) {
      const int k = base + u * 64 + lane;
      const int e = q[u].on ? trk_find(q[u].f, settled, key, S) : -1;
      int start = 0;
      if (e >= 0) start = wt[k].start;
      int64_t pos = -1;
      uint64_t todo = wv::ballot(e >= 0);
      while (todo) {
        const int lead = wv::ffs64(todo);
        const int el = wv::readlane(e, lead);
        const uint64_t m = wv::ballot(e == el);
        int old = 0;
        if (lane == lead) old = wv::atomic_add(&cur[el * WAVES + wave], wv::popc64(m));
        const int first = wv::readlane(old, lead);
        if (e == el) pos = (int64_t)first + wv::popc64(m & ((1ull << lane) - 1ull));
        todo &= ~m;
      }
      if (pos >= 0 && pos < a.cap) {
        rfid_tag_read r;
        r.stream = s; r.entry = e; r.seq = k; r.start = start;
        r.h_re = wv::u2f((uint32_t)q[u].h_re); r.h_im = wv::u2f((uint32_t)q[u].h_im); r.T = wv::u2f((uint32_t)q[u].T);
        r.index = q[u].index;
        a.out[pos] = r;
      }
    }
  }
}

}  // namespace rfidk
