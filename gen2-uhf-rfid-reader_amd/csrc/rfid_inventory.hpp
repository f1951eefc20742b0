// rfid_inventory.hpp -- the inventory stage of the batched path: per trace, one record (rfid_tag_entry) per DISTINCT
// 128-bit EPC frame among the CRC-verified reads before the TERMINATED cut-off -- the reads tag_reads[] counts
// (lib/tag_decoder_impl.cc:346-364, lib/gate_impl.cc:101-109), keyed by the whole frame instead of one byte of it.
// No counterpart in the reference: it is what a caller would otherwise compute on the host from every
// rfid_decode_result of a pass.
//
// Everything here is order-independent: integer atomic_add / atomic_min / atomic_max on LDS words and nothing else is
// shared between lanes, so a result does not depend on which wave got where first and a pass repeats bit for bit.  Only
// primitives both device environments offer (csrc/rfid_device_env.h and the wave emulator's): no compare-and-swap, no
// 64-bit maximum.
//
// The table.  `slots` (a power of two) words `owner[]` per trace, all INT_MAX at first.  A frame's probe sequence is
// slot_i = (h0 + i * step) & (slots - 1) with h0 and an ODD step hashed from its four words: `slots` probes visit every
// slot.  A slot is claimed for good by the EARLIEST read that asks for it while it is empty -- that read is the first
// read of its frame, which is why an entry's first_seq is its slot's owner and why no key needs a compare-and-swap: the
// key is copied from the owner's result once the slot is settled.  Rounds make that race-free:
//   round r: every read walks its probes 0..r over `settled[]` (the owners as they stood when the round began: nothing
//   writes it during a round).  A slot owned by its own frame: resolved.  A slot owned by another frame: next probe.
//   An empty slot (only ever its probe r): atomic_min(&owner[slot], window index) -- all reads that see the slot empty
//   contend in the same round, and min() does not care in which order.  After a workgroup barrier the owners are copied
//   to settled[] with their keys, and the next round begins.
// All reads of one frame see the same settled[] and walk the same probes, so they end in the same slot.  Every round
// that is not the last settles at least one more slot or moves the unresolved reads one probe on; after `slots` probes a
// read has seen every slot, so slots + 1 rounds at most -- a trace with more distinct frames than slots (or than
// max_tags) sets its overflow flag and lists nothing.  With the default table (>= 2 x max_tags slots) two rounds are the
// rule: one that claims, one in which every read finds its frame.
// Counts, last read and the largest |h|^2 are accumulated by the reads that resolve in a round and thrown away if the
// round turns out not to be the last; the strongest read's seq needs the maximum first and takes one more walk.
//
// Also here, because the tracks stage (rfid_tracks.hpp, which includes this file) decides the same thing: inv_hash / inv_walk
// (how a frame is looked up in the table).  How a table is BUILT is not shared: reads claim slots here, entries in the tracks.
// What all stages share -- stage_windows, stage_fetch, scan_share / scan_partials -- is in rfid_stage.hpp.
#pragma once
#include "rfid_stage.hpp"

namespace rfidk {

struct InvArgs {
  const rfid_decode_result *res;    // [n_streams][wmax]
  const int *wcount;                // [n_streams]
  const rfid_stream_stats *stats;   // [n_streams]: n_windows_used of the same pass
  int wmax, n_streams;
  int max_tags;                     // rows of `out` per trace
  int slots;                        // power of two, 2 .. SLOTS of the instantiation
  rfid_tag_entry *out;              // [n_streams][max_tags], ordered by first_seq
  int *counts;                      // [n_streams]: entries written (0 when the trace overflowed)
  int *overflow;                    // [n_streams]: 1 = more distinct frames than max_tags (or than slots)
};

constexpr int INV_EMPTY = 0x7fffffff;
constexpr int INV_MAX_WAVES = 16;
constexpr int INV_UNROLL = 4;       // 64-window batches of loads in flight per wave

// int pattern of h_re*h_re + h_im*h_im (non-negative: ordered like the float)
RFID_DEVICE int inv_norm(const StageRead &q) {
  const float re = wv::u2f((uint32_t)q.h_re), im = wv::u2f((uint32_t)q.h_im);
  const float n = re * re + im * im;              // (binary32, two products and one sum: -ffp-contract=off)
  return (int)(wv::f2u(n) & 0x7fffffffu);
}

RFID_DEVICE void inv_hash(const uint32_t (&f)[4], int mask, int &h0, int &step) {
  uint32_t h = (f[0] * 0x9E3779B1u) ^ (f[1] * 0x85EBCA77u) ^ (f[2] * 0xC2B2AE3Du) ^ (f[3] * 0x27D4EB2Fu);
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  h0 = (int)(h & (uint32_t)mask);
  step = (int)(((h >> 16) & (uint32_t)mask) | 1u);
}

// the slot among probes 0..last whose settled owner holds this frame: its index, -1 when an empty slot comes first
// (`empty_slot` names it), -2 when every probe is owned by another frame
RFID_DEVICE int inv_walk(const uint32_t (&f)[4], const int *settled, const uint32_t *key, int mask, int last, int &empty_slot) {
  int h0, step;
  inv_hash(f, mask, h0, step);
  for (int i = 0; i <= last; ++i) {
    const int slot = (h0 + i * step) & mask;
    if (settled[slot] == INV_EMPTY) { empty_slot = slot; return -1; }
    const uint32_t *kk = key + 4 * slot;
    if (kk[0] == f[0] && kk[1] == f[1] && kk[2] == f[2] && kk[3] == f[3]) return slot;
  }
  return -2;
}

// One workgroup per trace: one wavefront, or sixteen when a trace can hold thousands of windows (the host picks, as for
// stream_stats_kernel).  Every pass over the windows keeps INV_UNROLL batches of 64 results in flight per wave.
template <int SLOTS>
RFID_KERNEL(64 * INV_MAX_WAVES) void inventory_kernel(InvArgs a) {
  RFID_SHARED int owner[SLOTS];
  RFID_SHARED int settled[SLOTS];
  RFID_SHARED uint32_t key[4 * SLOTS];
  RFID_SHARED int cnt[SLOTS];
  RFID_SHARED int last[SLOTS];
  RFID_SHARED int bestn[SLOTS];
  RFID_SHARED int bests[SLOTS];
  RFID_SHARED int sh_again, sh_n;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const int s = (int)blockIdx.x;
  if (s >= a.n_streams) return;
  const int S = a.slots, mask = S - 1;
  for (int i = tid; i < S; i += nthr) {
    owner[i] = INV_EMPTY; settled[i] = INV_EMPTY;
    cnt[i] = 0; last[i] = -1; bestn[i] = -1; bests[i] = INV_EMPTY;
  }
  if (tid == 0) { sh_again = 0; sh_n = 0; }
  wv::block_sync();
  const int nw = stage_windows(a.wcount, a.stats, a.wmax, s);
  const rfid_decode_result *rs = a.res + (int64_t)s * a.wmax;
  bool full = false;     // more distinct frames than slots
  for (int r = 0;; ++r) {
    const int deepest = (r < S) ? r : (S - 1);
    for (int base = 0; base < nw; base += nthr * INV_UNROLL) {
      StageRead q[INV_UNROLL];
#pragma unroll
      for (int u = 0; u < INV_UNROLL; ++u) q[u] = stage_fetch(rs, base + u * nthr + tid, nw);
#pragma unroll
      for (int u = 0; u < INV_UNROLL; ++u) {
        if (!q[u].on) continue;
        const int k = base + u * nthr + tid;
        int empty_slot = 0;
        const int slot = inv_walk(q[u].f, settled, key, mask, deepest, empty_slot);
        if (slot >= 0) {
          wv::atomic_add(&cnt[slot], 1);
          wv::atomic_max(&last[slot], k);
          wv::atomic_max(&bestn[slot], inv_norm(q[u]));
        } else {
          if (slot == -1) wv::atomic_min(&owner[empty_slot], k);
          sh_again = 1;     // (every writer stores the same value)
        }
      }
    }
    wv::block_sync();
    const bool again = sh_again != 0;
    if (!again) break;
    if (r >= S) { full = true; break; }     // (every read has seen every slot)
    wv::block_sync();                       // (all have read sh_again)
    for (int i = tid; i < S; i += nthr) {
      const int o = owner[i];
      if (o != settled[i]) {
        settled[i] = o;
        key[4 * i + 0] = rs[o].bits[0]; key[4 * i + 1] = rs[o].bits[1];
        key[4 * i + 2] = rs[o].bits[2]; key[4 * i + 3] = rs[o].bits[3];
      }
      cnt[i] = 0; last[i] = -1; bestn[i] = -1;
    }
    if (tid == 0) sh_again = 0;
    wv::block_sync();
  }
  // distinct frames
  for (int i = tid; i < S; i += nthr)
    if (settled[i] != INV_EMPTY) wv::atomic_add(&sh_n, 1);
  wv::block_sync();
  const int n_ent = sh_n;
  if (full || n_ent > a.max_tags) {
    if (tid == 0) { a.counts[s] = 0; a.overflow[s] = 1; }
    return;
  }
  // the strongest read of every frame: the earliest among those that hold the maximum
  for (int base = 0; base < nw; base += nthr * INV_UNROLL) {
    StageRead q[INV_UNROLL];
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) q[u] = stage_fetch(rs, base + u * nthr + tid, nw);
#pragma unroll
    for (int u = 0; u < INV_UNROLL; ++u) {
      if (!q[u].on) continue;
      int empty_slot = 0;
      const int slot = inv_walk(q[u].f, settled, key, mask, S - 1, empty_slot);
      if (slot >= 0 && inv_norm(q[u]) == bestn[slot]) wv::atomic_min(&bests[slot], base + u * nthr + tid);
    }
  }
  wv::block_sync();
  // entries in the order of their first reads: an entry's place is the number of earlier owners
  rfid_tag_entry *out = a.out + (int64_t)s * a.max_tags;
  for (int i = tid; i < S; i += nthr) {
    const int o = settled[i];
    if (o == INV_EMPTY) continue;
    int rank = 0;
    for (int j = 0; j < S; ++j) rank += (settled[j] < o) ? 1 : 0;
    if (rank >= a.max_tags) continue;     // (not reached: n_ent <= max_tags)
    const int b = bests[i];
    rfid_tag_entry e;
    e.stream = s; e.reads = cnt[i];
    e.frame[0] = key[4 * i + 0]; e.frame[1] = key[4 * i + 1]; e.frame[2] = key[4 * i + 2]; e.frame[3] = key[4 * i + 3];
    e.first_seq = o; e.last_seq = last[i]; e.best_seq = b;
    e.best_h_re = rs[b].h_re; e.best_h_im = rs[b].h_im;
    e.tag_id = rs[o].tag_id;
    out[rank] = e;
  }
  if (tid == 0) { a.counts[s] = n_ent; a.overflow[s] = 0; }
}

// ---- the entries of all traces in one piece: offsets (one workgroup), then the copy ----------------------------------
struct InvPackArgs {
  const rfid_tag_entry *in;     // [n_streams][max_tags]
  const int *counts, *overflow; // [n_streams]
  int n_streams, max_tags;
  int *offsets;                 // [n_streams]: entries of the traces before this one
  int *head;                    // [0] entries in all, [1] the first trace that overflowed (INV_EMPTY: none)
  rfid_tag_entry *packed;       // [sum of counts]
};

RFID_KERNEL(INV_SCAN_THREADS) void inventory_offsets_kernel(InvPackArgs a) {
  RFID_SHARED int part[INV_SCAN_THREADS];
  RFID_SHARED int sh_over;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  if (tid == 0) sh_over = INV_EMPTY;
  wv::block_sync();
  const ScanShare sh = scan_share(a.n_streams, tid, nthr);
  int sum = 0, over = INV_EMPTY;
  for (int b = sh.b0; b < sh.b1; ++b) {
    sum += a.counts[b];
    if (a.overflow[b] && b < over) over = b;
  }
  if (over != INV_EMPTY) wv::atomic_min(&sh_over, over);
  int total = 0;
  int run = scan_partials(part, tid, nthr, sum, total);
  if (tid == 0) { a.head[0] = total; a.head[1] = sh_over; }
  for (int b = sh.b0; b < sh.b1; ++b) { a.offsets[b] = run; run += a.counts[b]; }
}

RFID_KERNEL(64) void inventory_pack_kernel(InvPackArgs a) {
  constexpr int WORDS = (int)(sizeof(rfid_tag_entry) / sizeof(int));
  const int s = (int)blockIdx.x;
  if (s >= a.n_streams) return;
  const int n = a.counts[s] * WORDS;
  const int *src = reinterpret_cast<const int *>(a.in + (int64_t)s * a.max_tags);
  int *dst = reinterpret_cast<int *>(a.packed + a.offsets[s]);
  for (int w = (int)threadIdx.x; w < n; w += (int)blockDim.x) dst[w] = src[w];
}

}  // namespace rfidk
