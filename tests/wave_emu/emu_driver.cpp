// tests/wave_emu/emu_driver.cpp -- TEST INFRASTRUCTURE ONLY (see rfid_device_env.h here).
//
// Runs the unmodified kernel source gen2-uhf-rfid-reader_amd/csrc/rfid_kernels.hpp on a
// lock-step 64-lane host emulator so the kernel logic (indices, state machine, ring
// handling, reductions) can be compared with the oracle in the GPU-less CI container.
// Built by tests/wave_emu/build.py into tests/wave_emu/librfid_wave_emu.so (and, with the
// device's LS2_FIN_WPB = 1, librfid_wave_emu_wpb1.so); nothing in the product imports or links it.
// How the workgroups of a launch are run (one at a time, or resident at once under a seeded
// schedule) is emu_schedule()'s: see emu::launch below.
#include <stdio.h>
#include <stdlib.h>

#include <semaphore.h>
#include <sys/mman.h>

#include <algorithm>
#include <functional>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <rfid_device_env.h>
#include "rfid_host_math.h"
#include "rfid_kernels.hpp"
#include "rfid_tracks.hpp"   // (and through it rfid_inventory.hpp, rfid_stage.hpp)
#include "rfid_gen2_host.h"
#define LS2_DCB_SNAPS_N 2   // (a unit's gate openings go through LDS two at a time here: the in-between writes are exercised)
#ifndef LS2_FIN_WPB       // (build.py builds both: 16 -- the finishing walk's waves of a trace share one workgroup by default, or two and
#define LS2_FIN_WPB 16    // more with ls2_fin_waves_force() -- and the device's 1, one-wave workgroups that meet, under a concurrent schedule)
#endif
#define LS2_LAUNCH(kernel, gx, gy, block, args) \
  emu::launch(emu::Idx3{(unsigned)(gx), (unsigned)(gy), 1}, emu::Idx3{(unsigned)(block), 1, 1}, [&]() { rfidk::kernel(args); }, #kernel)
#include "rfid_ls2_enqueue.hpp"

namespace emu {

thread_local Block *g_blk = nullptr;
thread_local Fiber *g_cur = nullptr;
thread_local Idx3 g_block_idx, g_grid_dim, g_block_dim;
thread_local ucontext_t g_sched;
static thread_local const std::function<void()> *g_body = nullptr;

void yield() { swapcontext(&g_cur->ctx, &g_sched); }

static void fiber_entry() {
  (*g_body)();
  g_cur->done = true;
  swapcontext(&g_cur->ctx, &g_sched);
}

// ---- schedules ----
// 0: one workgroup at a time in index order, on the calling thread (the default).  The others keep every workgroup of a launch
// resident at once (up to RESIDENT_LANES lanes; the rest is dispatched in order as workgroups finish), each on a thread of its own:
// 1 in order (the lowest-index workgroup that can make progress runs), 2 reversed (the highest), 3 random (a seeded pick among the
// workgroups that can make progress, after every wave-level step), 4 late dispatch (as 1, but the lower half of each trace's
// workgroups -- blockIdx.x < gridDim.x / 2; the upper half for an odd seed -- is dispatched only once all the others wait or are done)
enum { SCHED_SEQ = 0, SCHED_IN_ORDER = 1, SCHED_REVERSED = 2, SCHED_RANDOM = 3, SCHED_LATE = 4 };
static int g_kind = SCHED_SEQ;
static uint64_t g_seed = 0, g_launch_no = 0;
constexpr size_t STACK = 256 * 1024;          // per fiber: reserved, committed as it is touched
// lanes resident at once under the concurrent schedules: 256 one-wave workgroups (a quarter of the finishing walk's 1 024 on the
// device -- each resident workgroup is a thread with its own copy of every kernel's LDS).  A launch whose workgroups must all be
// resident to finish (the walk with G x B > 256) is reported as a deadlock, naming how many were resident
constexpr int RESIDENT_LANES = 16384;
constexpr int MAX_SLOTS = 256;
// wave-level steps (sweeps) one workgroup may take under the concurrent schedules before its launch is reported as one that does not
// end (a livelock: a workgroup that keeps going without ever waiting, e.g. on records no other workgroup will write).  The longest
// workgroup of the suite's concurrent runs takes some 5 000 (50 x less)
static long g_sweep_limit = 250000;
static bool g_failed = false;                 // a launch deadlocked or did not end: the launches behind it in the run return at once
static std::string g_error;

// a resident workgroup: its fibers with their stacks and, under the concurrent schedules, the OS thread that runs them
struct Slot {
  Block B;
  char *stacks = nullptr;
  size_t n_stacks = 0;
  Idx3 grid, block, idx;
  const std::function<void()> *body = nullptr;
  long sweeps = 0;
  bool live = false;
  uint64_t stalled_at = ~0ull;      // the scheduler's epoch at its last step without progress
  // hand-off (concurrent schedules)
  std::thread th;
  sem_t go;
  int cmd = 0, quantum = 1;
  bool progressed = false;
};
static sem_t g_back;
static std::vector<Slot *> g_pool;

static void ensure_stacks(Slot &S, size_t n) {
  if (n <= S.n_stacks) return;
  if (S.stacks) munmap(S.stacks, S.n_stacks * STACK);
  void *p = mmap(nullptr, n * STACK, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (p == MAP_FAILED) { perror("[emu] fiber stacks"); abort(); }
  S.stacks = (char *)p;
  S.n_stacks = n;
}

// (on the slot's own thread: the thread-local state is that thread's)
static void start_wg(Slot &S) {
  g_grid_dim = S.grid; g_block_dim = S.block; g_block_idx = S.idx; g_body = S.body;
  const int nthreads = (int)(S.block.x * S.block.y * S.block.z), nwaves = (nthreads + 63) / 64;
  Block &B = S.B;
  ensure_stacks(S, (size_t)nthreads);
  B.nthreads = nthreads;
  B.fibers.resize((size_t)nthreads);
  B.xbuf.assign((size_t)nwaves * 2 * 64, 0);
  B.wave_arrived.assign((size_t)nwaves, 0);
  B.wave_gen.assign((size_t)nwaves, 0);
  B.block_arrived = 0;
  B.block_gen = 0;
  for (int t = 0; t < nthreads; ++t) {
    Fiber &f = B.fibers[(size_t)t];
    f.stack = S.stacks + (size_t)t * STACK;
    f.tid = Idx3{(unsigned)t, 0, 0};
    f.done = false;
    f.wave_calls = f.block_calls = f.grid_calls = 0;
    f.at = "start";
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = f.stack;
    f.ctx.uc_stack.ss_size = STACK;
    f.ctx.uc_link = &g_sched;
    makecontext(&f.ctx, fiber_entry, 0);
  }
  S.sweeps = 0;
  S.live = true;
}

// every live fiber of the workgroup once; -> whether any of them got further than re-checking its wait condition
static bool sweep(Slot &S) {
  Block &B = S.B;
  g_blk = &B;
  const int nthreads = B.nthreads, nwaves = (nthreads + 63) / 64;
  // watchdog (a kernel that never finishes under lock-step emulation): report where the waves stand
  if (++S.sweeps == 3000000L && getenv("RFID_EMU_WATCHDOG")) {
    for (int w = 0; w < nwaves; ++w) {
      const Fiber &f0 = B.fibers[(size_t)w * 64];
      fprintf(stderr, "[emu watchdog] wave %d: lane0 done=%d wave_calls=%llu arrived=%d gen=%llu", w, (int)f0.done,
              (unsigned long long)f0.wave_calls, B.wave_arrived[(size_t)w], (unsigned long long)B.wave_gen[(size_t)w]);
      for (int l = 1; l < 64 && w * 64 + l < nthreads; ++l)
        if (B.fibers[(size_t)w * 64 + l].wave_calls != f0.wave_calls || B.fibers[(size_t)w * 64 + l].done != f0.done) {
          fprintf(stderr, " | lane %d: done=%d wave_calls=%llu", l, (int)B.fibers[(size_t)w * 64 + l].done,
                  (unsigned long long)B.fibers[(size_t)w * 64 + l].wave_calls);
          break;
        }
      fprintf(stderr, "\n");
    }
    abort();
  }
  bool moved = false;
  int remaining = 0;
  for (int t = 0; t < nthreads; ++t) {
    Fiber &f = B.fibers[(size_t)t];
    if (f.done) continue;
    const uint64_t p0 = f.position();
    g_cur = &f;
    swapcontext(&g_sched, &f.ctx);
    if (f.position() != p0) moved = true;
    if (!f.done) remaining++;
  }
  g_blk = nullptr;
  g_cur = nullptr;
  S.live = remaining > 0;
  return moved;
}

static void slot_main(Slot *S) {
  for (;;) {
    sem_wait(&S->go);
    if (S->cmd == 0) {
      start_wg(*S);
      S->progressed = true;
    } else {
      bool any = false;
      for (int q = 0; q < S->quantum; ++q) {
        const bool m = sweep(*S);
        any = any || m;
        if (!m || !S->live) break;
      }
      S->progressed = any;
    }
    sem_post(&g_back);
  }
}

static Slot *pool_slot(size_t k) {
  if (g_pool.empty()) sem_init(&g_back, 0, 0);
  while (g_pool.size() <= k) {
    Slot *S = new Slot;
    sem_init(&S->go, 0, 0);
    S->th = std::thread(slot_main, S);
    S->th.detach();
    g_pool.push_back(S);
  }
  return g_pool[k];
}
static void on_slot(Slot *S, int cmd, int quantum) {
  S->cmd = cmd; S->quantum = quantum;
  sem_post(&S->go);
  sem_wait(&g_back);
}

static void report_deadlock(const char *name, Idx3 grid, Idx3 block, const std::vector<Slot *> &stuck, const char *why = nullptr) {
  char line[512];
  snprintf(line, sizeof(line), "%s in %s (grid %u x %u, %u threads): %s --", why ? "no end" : "deadlock", name, grid.x, grid.y, block.x,
           why ? why : "every live workgroup waits");
  std::string m = line;
  int shown = 0;
  for (const Slot *S : stuck) {
    if (shown++ == 24) { m += " ..."; break; }
    const Fiber *f0 = nullptr;
    int live = 0;
    for (const Fiber &f : S->B.fibers) if (!f.done) { live++; if (!f0) f0 = &f; }
    snprintf(line, sizeof(line), " wg (%u,%u): %d lanes live, lane %u at %s (wave ops %llu, block syncs %llu, grid waits %llu);",
             S->idx.x, S->idx.y, live, f0 ? f0->tid.x : 0u, f0 ? f0->at : "-", f0 ? (unsigned long long)f0->wave_calls : 0ull,
             f0 ? (unsigned long long)f0->block_calls : 0ull, f0 ? (unsigned long long)f0->grid_calls : 0ull);
    m += line;
  }
  g_error = m;
  g_failed = true;
}

static Slot g_seq_slot;   // (schedule 0: on the calling thread)

void launch(Idx3 grid, Idx3 block, const std::function<void()> &body, const char *name) {
  if (g_failed) return;
  const long total = (long)grid.x * grid.y * grid.z;
  if (total <= 0) return;
  auto idx_of = [&](long i) { return Idx3{(unsigned)(i % grid.x), (unsigned)((i / grid.x) % grid.y), (unsigned)(i / ((long)grid.x * grid.y))}; };
  if (g_kind == SCHED_SEQ) {
    Slot &S = g_seq_slot;
    S.grid = grid; S.block = block; S.body = &body;
    for (long i = 0; i < total; ++i) {
      S.idx = idx_of(i);
      start_wg(S);
      while (S.live)
        if (!sweep(S) && S.live) {   // (nothing else runs: it waits for ever)
          report_deadlock(name, grid, block, std::vector<Slot *>{&S});
          S.live = false;
          return;
        }
    }
    return;
  }
  const int nthreads = (int)(block.x * block.y * block.z);
  int cap = RESIDENT_LANES / (nthreads > 0 ? nthreads : 1);
  cap = cap < 1 ? 1 : (cap > MAX_SLOTS ? MAX_SLOTS : cap);
  std::mt19937_64 rng(g_seed * 0x9E3779B97F4A7C15ull + (++g_launch_no));
  // dispatch order; late: held back until every dispatched workgroup waits or is done
  std::vector<long> pending, late;
  for (long j = 0; j < total; ++j) {
    const long i = j;   // (dispatch is in index order, as the device's; `reversed` runs the highest-index RESIDENT workgroup first)
    const unsigned x = idx_of(i).x;
    if (g_kind == SCHED_LATE && grid.x >= 2 && ((g_seed & 1) ? x >= (grid.x + 1) / 2 : x < grid.x / 2)) late.push_back(i);
    else pending.push_back(i);
  }
  size_t next = 0;
  bool late_released = false;
  std::vector<Slot *> active, free_slots;
  for (int k = cap - 1; k >= 0; --k) free_slots.push_back(pool_slot((size_t)k));
  uint64_t epoch = 0;
  const int quantum = (g_kind == SCHED_RANDOM) ? 1 : 256;
  for (;;) {
    while (!free_slots.empty() && next < pending.size()) {
      Slot *S = free_slots.back();
      free_slots.pop_back();
      S->grid = grid; S->block = block; S->body = &body; S->idx = idx_of(pending[next++]);
      S->stalled_at = ~0ull;
      on_slot(S, 0, 0);
      active.push_back(S);
      epoch++;
    }
    if (active.empty() && next == pending.size()) {
      if (late_released || late.empty()) break;
    }
    std::vector<Slot *> can;
    for (Slot *S : active) if (S->stalled_at != epoch) can.push_back(S);
    if (can.empty()) {
      if (!late_released && !late.empty()) {
        late_released = true;
        pending.insert(pending.end(), late.begin(), late.end());
        continue;
      }
      report_deadlock(name, grid, block, active);
      if (next < pending.size()) {   // (residency: the workgroups that would have let them go on were never dispatched)
        char why[160];
        snprintf(why, sizeof(why), " [%zu of the launch's %ld workgroups resident, at most %d at once]", active.size(), total, cap);
        g_error += why;
      }
      for (Slot *S : active) S->live = false;
      return;
    }
    Slot *S = (g_kind == SCHED_RANDOM) ? can[(size_t)(rng() % can.size())] : (g_kind == SCHED_REVERSED) ? can.back() : can.front();
    on_slot(S, 1, quantum);
    if (S->progressed) epoch++;
    else S->stalled_at = epoch;
    if (S->live && S->sweeps >= g_sweep_limit) {
      char why[200];
      snprintf(why, sizeof(why), "workgroup (%u,%u) took %ld wave-level steps without finishing (limit %ld)", S->idx.x, S->idx.y, S->sweeps,
               g_sweep_limit);
      report_deadlock(name, grid, block, active, why);
      for (Slot *R : active) R->live = false;
      return;
    }
    if (!S->live) {
      active.erase(std::find(active.begin(), active.end(), S));
      free_slots.push_back(S);
    }
  }
}

}  // namespace emu

using namespace rfidk;

constexpr int EMU_DEADLOCK = -100;   // a launch of the run deadlocked or did not end (emu_last_error says where)
// every entry point that launches starts a run: no failure of an earlier run carries over, and the schedule depends on the seed alone
struct EmuRun {
  EmuRun() { emu::g_failed = false; emu::g_launch_no = 0; }
  int rc(int ok) const { return emu::g_failed ? EMU_DEADLOCK : ok; }
};

extern "C" {

// Batched pipeline mf -> gate -> decode -> stats, mirroring rfid_batch_process().
// raw: [B][stride] complex64.  Outputs ordered by (stream, seq).
int emu_batch_process(const float *raw, int B, long stride, long n_raw, const int64_t *lens, int fixed_q,
                      int max_num_queries, int number_unique_tags, rfid_window *windows,
                      rfid_decode_result *results, rfid_scores *scores, long cap, long *n_windows,
                      rfid_stream_stats *stats, float *y_out, long gate_chunk) {
  EmuRun run;
  const long n_dec = n_raw / DECIM;
  long y_stride = (n_dec + 1) & ~1L;
  if (y_stride < 2) y_stride = 2;
  std::vector<float4> ybuf((size_t)(y_stride * B / 2 + 2));
  float2 *y = reinterpret_cast<float2 *>(ybuf.data());
  const int wmax = (int)(n_dec / (RN16_WIN + T1_SAMPLES + 1) + 2);
  const int flat_cap = wmax * B;
  std::vector<GateState> gstate((size_t)B);
  memset(gstate.data(), 0, sizeof(GateState) * (size_t)B);
  std::vector<rfid_window> wtab((size_t)flat_cap), flat((size_t)flat_cap * 2);
  std::vector<int> wcount((size_t)B, 0);
  int flat_count[2] = {0, 0};
  std::vector<rfid_decode_result> res((size_t)flat_cap);
  std::vector<rfid_scores> sc((size_t)flat_cap);
  memset(sc.data(), 0, sizeof(rfid_scores) * (size_t)flat_cap);

  MfArgs ma;
  ma.x = reinterpret_cast<const float2 *>(raw); ma.x_stride = stride; ma.n_raw = n_raw; ma.lens = lens;
  ma.n_out = n_dec; ma.in_off = -(NTAPS - 1);
  ma.vec_ok = ((stride & 1) == 0 && (((uintptr_t)raw) & 15) == 0) ? 1 : 0;
  ma.y = y; ma.y_stride = y_stride; ma.tile0 = 0; ma.stream0 = 0;
  const long tiles = (n_dec + MF_TILE - 1) / MF_TILE;
  const bool fused = gate_chunk < 0;   // gate_chunk -1: the fused front end, as rfid_batch_process() runs by default
  if (tiles > 0 && !fused)
    emu::launch(emu::Idx3{(unsigned)tiles, (unsigned)B, 1}, emu::Idx3{MF_THREADS, 1, 1},
                [&]() { mf_boxcar25_decim5_kernel(ma); });

  GateArgs ga = {};
  ga.y = y; ga.y_stride = y_stride; ga.n_dec = n_dec; ga.lens = lens; ga.state = gstate.data(); ga.n_streams = B;
  ga.wtab = wtab.data(); ga.wmax = wmax; ga.wcount = wcount.data(); ga.flat = flat.data();
  ga.flat_count = flat_count; ga.flat_cap = flat_cap; ga.mode = 0; ga.gated = nullptr; ga.gated_cap = 0;
  ga.io = nullptr;
  if (fused) {
    ga.pos0 = 0; ga.chunk_len = n_dec; ga.y_w = y;
    ga.raw = reinterpret_cast<const float2 *>(raw); ga.raw_stride = stride; ga.n_raw = n_raw; ga.raw_vec_ok = ma.vec_ok;
    emu::launch(emu::Idx3{(unsigned)((B + GATE_STREAMS_PER_WG - 1) / GATE_STREAMS_PER_WG), 1, 1},
                emu::Idx3{GATE_THREADS, 1, 1}, [&]() { front_end_fused_kernel(ga); });
  } else {
    // time-chunked launches with carried state, as rfid_batch_process() issues them
    const long chunk = (gate_chunk > 0) ? gate_chunk : (n_dec > 0 ? n_dec : 1);
    for (long p0 = 0; p0 == 0 || p0 < n_dec; p0 += chunk) {
      ga.pos0 = p0; ga.chunk_len = chunk;
      emu::launch(emu::Idx3{(unsigned)((B + GATE_STREAMS_PER_WG - 1) / GATE_STREAMS_PER_WG), 1, 1},
                  emu::Idx3{GATE_THREADS, 1, 1}, [&]() { gate_scan_kernel(ga); });
    }
  }
  if (y_out)
    for (int b = 0; b < B; ++b) memcpy(y_out + 2 * (size_t)b * n_dec, y + (size_t)b * y_stride, sizeof(float2) * (size_t)n_dec);

  DecodeListArgs da;
  da.y = y; da.y_stride = y_stride; da.cap = flat_cap; da.res = res.data(); da.scores = sc.data(); da.wmax = wmax;
  da.sum = nullptr;   // (the statistics kernel reads the results themselves here; emu_ls2_process runs it on the one-word summaries)
  rfidh::t_candidates(da.t_cand, 400000);
  {   // the one-launch tag_decoder, as rfid_batch_decode launches it (2 persistent waves here)
    DecodeAllArgs all;
    int ticket = 0, ticket_next = 0;
    all.epc = da; all.rn16 = da; all.ticket = &ticket; all.ticket_next = &ticket_next;
    all.epc.list = flat.data() + flat_cap; all.epc.count = &flat_count[1];
    all.rn16.list = flat.data(); all.rn16.count = &flat_count[0];
    emu::launch(emu::Idx3{2, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { decode_all_kernel(all); });
  }

  StatsArgs sa;
  sa.res = res.data(); sa.wcount = wcount.data(); sa.wmax = wmax; sa.n_streams = B;
  sa.max_slot_number = 1 << fixed_q; sa.max_num_queries = max_num_queries;
  sa.number_unique_tags = number_unique_tags; sa.out = stats; sa.sum = nullptr;
  emu::launch(emu::Idx3{(unsigned)B, 1, 1}, emu::Idx3{256, 1, 1}, [&]() { stream_stats_kernel(sa); });   // four waves share a trace's windows

  long total = 0;
  for (int s = 0; s < B; ++s) {
    for (int k = 0; k < wcount[(size_t)s]; ++k) {
      if (total < cap) {
        const size_t off = (size_t)s * (size_t)wmax + (size_t)k;
        if (windows) windows[total] = wtab[off];
        if (results) results[total] = res[off];
        if (scores) scores[total] = sc[off];
      }
      total++;
    }
  }
  *n_windows = total;
  return run.rc(0);
}

// The long-stream front end (rfid_ls2.hpp) in place of the sequential gate scan: mf -> pieces / avg_ampl / state machine /
// dc_est / windows (the launch list of rfid_ls2_enqueue.hpp, as the library enqueues it) -> the sequential scan as the
// skipped-or-not fallback -> decode -> stats.  min_piece / target shrink the pieces so that small traces are cut many
// times.  cuts: test hook -- the idle-cut search is replaced by these positions (trace 0).  ctl_out: the Ls2Ctl block as ints.  carry / hold_last = the streaming form (state_blob: GateState of trace 0 in
// and out, consumed[0] = first unprocessed sample).
int emu_ls2_process(const float *raw, int B, long stride, long n_raw, const int64_t *lens, int fixed_q,
                    int max_num_queries, int number_unique_tags, rfid_window *windows,
                    rfid_decode_result *results, rfid_scores *scores, long cap, long *n_windows,
                    rfid_stream_stats *stats, int min_piece, int target, int *ctl_out, int ctl_cap,
                    void *state_blob, int hold_last, int *consumed_out, int *pieces_out, int pieces_cap,
                    const int *cuts, int n_cuts, int y_skip, int generous, int dc_rounds, int fused) {
  EmuRun run;
  const long n_dec_all = n_raw / DECIM;
  const long n_dec = n_dec_all - y_skip;   // (y_skip: leading outputs that only exist to give the filter its history)
  long y_stride = (n_dec_all + 1) & ~1L;
  if (y_stride < 2) y_stride = 2;
  std::vector<float4> ybuf((size_t)(y_stride * B / 2 + 2));
  float2 *y0 = reinterpret_cast<float2 *>(ybuf.data());
  float2 *y = y0 + y_skip;
  const int wmax = (int)(n_dec / (RN16_WIN + T1_SAMPLES + 1) + 2);
  const int flat_cap = wmax * B;
  std::vector<GateState> gstate((size_t)B);
  memset(gstate.data(), 0, sizeof(GateState) * (size_t)B);
  if (state_blob) memcpy(gstate.data(), state_blob, sizeof(GateState));
  std::vector<rfid_window> wtab((size_t)flat_cap), flat((size_t)flat_cap * 2);
  std::vector<int> wcount((size_t)B, 0);
  int flat_count[2] = {0, 0};
  std::vector<rfid_decode_result> res((size_t)flat_cap);
  std::vector<rfid_scores> sc((size_t)flat_cap);
  memset(sc.data(), 0, sizeof(rfid_scores) * (size_t)flat_cap);

  MfArgs ma;
  ma.x = reinterpret_cast<const float2 *>(raw); ma.x_stride = stride; ma.n_raw = n_raw; ma.lens = lens;
  ma.n_out = n_dec_all; ma.in_off = -(NTAPS - 1);
  ma.vec_ok = ((stride & 1) == 0 && (((uintptr_t)raw) & 15) == 0) ? 1 : 0;
  ma.y = y0; ma.y_stride = y_stride; ma.tile0 = 0; ma.stream0 = 0;
  const long tiles = (n_dec_all + MF_TILE - 1) / MF_TILE;
  // fused: the long-stream front end's first pass runs the matched filter itself (ls2_front_kernel), as rfid_batch_process does
  // for fresh traces; y is only filtered here when that pass is not taken or gives up
  auto run_mf = [&]() {
    if (tiles > 0)
      emu::launch(emu::Idx3{(unsigned)tiles, (unsigned)B, 1}, emu::Idx3{MF_THREADS, 1, 1}, [&]() { mf_boxcar25_decim5_kernel(ma); });
  };
  if (fused && (state_blob || hold_last || y_skip)) return -1;
  if (!fused) run_mf();

  const Ls2Geometry geo = ls2_geometry(B, n_dec, min_piece, target);
  std::vector<char> ws;
  Ls2Ctl ctl_host;
  memset(&ctl_host, 0, sizeof(ctl_host));
  int ok = 0;
  if (geo.P > 0) {
    const Ls2Layout L = ls2_layout(geo, B, y_stride, wmax);
    ws.assign(L.total + 256, 0);
    char *base = ws.data() + (256 - ((uintptr_t)ws.data() & 255));
    Ls2Args a;
    memset(&a, 0, sizeof(a));
    a.y = y; a.y_stride = y_stride; a.lens = lens; a.n_dec = n_dec; a.n_streams = B;
    ls2_bind(a, base, L, geo);
    a.wtab = wtab.data(); a.wmax = wmax; a.wcount = wcount.data(); a.flat = flat.data(); a.flat_count = flat_count; a.flat_cap = flat_cap;
    a.carry = state_blob ? gstate.data() : nullptr; a.carry_out = state_blob ? gstate.data() : nullptr;
    a.hold_last = hold_last; a.force = state_blob ? 1 : 0;
    if (fused) {
      a.fused = 1; a.raw = reinterpret_cast<const float2 *>(raw); a.raw_stride = stride; a.raw_vec_ok = ma.vec_ok; a.y_w = y;
    }
    if (cuts) {   // test hook: cut trace 0 at the given positions (ascending) instead of searching idle points
      for (int i = 0; i < B * geo.max_bc; ++i) a.cut[i] = -1;
      for (int k = 0; k < n_cuts; ++k) {   // (a cut stands for the grid point it lies behind, less than half a step away)
        const int J = cuts[k] / geo.Pc;
        if (J >= 1 && J < geo.max_bc && cuts[k] - J * geo.Pc < geo.Pc / 2) a.cut[J] = cuts[k];
      }
    }
    ls2_enqueue(a, cuts == nullptr, nullptr, generous != 0, dc_rounds);
    ctl_host = *a.ctl;
    ok = a.ctl->ok;
    if (consumed_out) consumed_out[0] = a.consumed[0];
    if (pieces_out) {   // per piece in use: trace, pos0, len, true start of avg_ampl / dc_est (bit patterns), unit head
      int k = 0;
      for (int i = 0; i < geo.NS && k < pieces_cap; ++i) {
        if (a.piece[i].len <= 0) continue;
        int *o = pieces_out + 8 * k++;
        o[0] = i / geo.max_b; o[1] = a.piece[i].pos0; o[2] = a.piece[i].len;
        float f = ls2_from_ord(a.aT[i]); memcpy(&o[3], &f, 4);
        if (fused) { o[4] = o[5] = 0; o[6] = -1; o[7] = i; continue; }   // (the avg_ampl pieces are not the units' pieces there)
        const int h = a.fsm[i].unit;
        const int tu = (h / geo.max_b) * geo.max_bc + (h % geo.max_b) / LS2_FINE;   // the unit's idle-grid slot: its dc_est start
        f = ls2_from_ord(a.dT[2 * tu]); memcpy(&o[4], &f, 4);
        f = ls2_from_ord(a.dT[2 * tu + 1]); memcpy(&o[5], &f, 4);
        o[6] = h; o[7] = i;
      }
      if (k < pieces_cap) pieces_out[8 * k] = -1;
    }
  }
  if (ctl_out) memcpy(ctl_out, &ctl_host, sizeof(int) * (size_t)((int)(sizeof(Ls2Ctl) / 4) < ctl_cap ? (int)(sizeof(Ls2Ctl) / 4) : ctl_cap));
  if (fused && geo.P == 0) run_mf();
  if (!ok && !hold_last) {   // the fallback the library enqueues behind the front end (GateArgs::skip_if)
    if (fused && geo.P > 0) run_mf();   // (the fused first pass may have given up half-way: the library filters again, MfArgs::skip_if)
    if (state_blob) gstate[0].win_seq = 0;   // (a call's windows are numbered from 0, as the front end numbers them)
    GateArgs ga = {};
    ga.y = y; ga.y_stride = y_stride; ga.n_dec = n_dec; ga.lens = lens; ga.state = gstate.data(); ga.n_streams = B;
    ga.wtab = wtab.data(); ga.wmax = wmax; ga.wcount = wcount.data(); ga.flat = flat.data();
    ga.flat_count = flat_count; ga.flat_cap = flat_cap; ga.mode = 0; ga.pos0 = 0; ga.chunk_len = n_dec;
    emu::launch(emu::Idx3{(unsigned)((B + GATE_STREAMS_PER_WG - 1) / GATE_STREAMS_PER_WG), 1, 1},
                emu::Idx3{GATE_THREADS, 1, 1}, [&]() { gate_scan_kernel(ga); });
  }
  if (state_blob) memcpy(state_blob, gstate.data(), sizeof(GateState));

  std::vector<float4> sums4((size_t)flat_cap / 4 + 2);   // (16-byte aligned: the statistics kernel's 16-byte loads)
  struct { int *p; int *data() { return p; } } sums = {reinterpret_cast<int *>(sums4.data())};
  DecodeListArgs da;
  da.y = y; da.y_stride = y_stride; da.cap = flat_cap; da.res = res.data(); da.scores = sc.data(); da.wmax = wmax;
  da.sum = sums.data();
  rfidh::t_candidates(da.t_cand, 400000);
  da.list = flat.data() + flat_cap; da.count = &flat_count[1];
  emu::launch(emu::Idx3{2, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { decode_epc3_kernel(da); });
  da.list = flat.data(); da.count = &flat_count[0];
  emu::launch(emu::Idx3{2, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { decode_rn16x4_kernel(da); });

  StatsArgs sa;
  sa.res = res.data(); sa.wcount = wcount.data(); sa.wmax = wmax; sa.n_streams = B;
  sa.max_slot_number = 1 << fixed_q; sa.max_num_queries = max_num_queries;
  sa.number_unique_tags = number_unique_tags; sa.out = stats; sa.sum = sums.data();
  emu::launch(emu::Idx3{(unsigned)B, 1, 1}, emu::Idx3{256, 1, 1}, [&]() { stream_stats_kernel(sa); });

  long total = 0;
  for (int s = 0; s < B; ++s) {
    for (int k = 0; k < wcount[(size_t)s]; ++k) {
      if (total < cap) {
        const size_t off = (size_t)s * (size_t)wmax + (size_t)k;
        if (windows) windows[total] = wtab[off];
        if (results) results[total] = res[off];
        if (scores) scores[total] = sc[off];
      }
      total++;
    }
  }
  *n_windows = total;
  return run.rc(ok);
}
int emu_ls2_ctl_words(void) { return (int)(sizeof(Ls2Ctl) / 4); }
// waves per trace of the finishing walk (0: as the library chooses; else a multiple of LS2_FIN_WPB)
void emu_ls2_fin_waves(int n) { ls2_fin_waves_force() = n; }
int emu_fin_wpb(void) { return LS2_FIN_WPB; }
// how the workgroups of a launch are run (rfid_device_env.h here; emu::launch): 0 one at a time in index order, 1 in order, 2
// reversed, 3 random, 4 late dispatch -- all of a launch's workgroups resident at once for 1 - 4
void emu_schedule(int kind, unsigned long long seed) { emu::g_kind = kind; emu::g_seed = seed; emu::g_launch_no = 0; }
// wave-level steps a workgroup may take under the concurrent schedules (emu::g_sweep_limit) -> the limit before
long emu_sweep_limit(long n) { const long o = emu::g_sweep_limit; if (n > 0) emu::g_sweep_limit = n; return o; }
// the report of the last launch that deadlocked (empty if none since the last run began) -> its length
int emu_last_error(char *buf, int cap) {
  if (cap > 0) { snprintf(buf, (size_t)cap, "%s", emu::g_failed ? emu::g_error.c_str() : ""); }
  return emu::g_failed ? (int)emu::g_error.size() : 0;
}
// self-test of the deadlock report: `gx` x `gy` one-wave workgroups meet twice (as the finishing walk does); with `leave` set the last
// workgroup of each row returns before the second meeting, so the others wait for ever (leave 2: it loops for ever instead).  out[gy][gx]: 1 per workgroup through
// both meetings.  -> 0, or EMU_DEADLOCK
int emu_grid_meet_selftest(int gx, int gy, int leave, int *out) {
  EmuRun run;
  std::vector<int> bar((size_t)gy, 0);
  emu::launch(emu::Idx3{(unsigned)gx, (unsigned)gy, 1}, emu::Idx3{64, 1, 1}, [&]() {
    const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
    int *counter = bar.data() + s;
    wv::block_sync();
    wv::grid_meet(counter, (int)gridDim.x, tid);
    wv::block_sync();
    if (leave == 1 && blockIdx.x == gridDim.x - 1) return;
    if (leave == 2 && blockIdx.x == gridDim.x - 1) for (;;) wv::wave_sync();   // (goes on for ever without waiting: no end)
    wv::grid_meet(counter, 2 * (int)gridDim.x, tid);
    wv::block_sync();
    if (tid == 0) out[(size_t)s * gx + blockIdx.x] = 1;
  }, "grid_meet_selftest");
  return run.rc(0);
}
// slots per workgroup of the chain launches (the library: 4096): small values make the emulated traces span several workgroups
void emu_ls2_chain_slots(int n) { ls2_chain_slots() = n; }
void emu_ls2_dcb_top_min(int n) { ls2_dcb_top_min() = n; }
void emu_ls2_dcb_bias(int n) { ls2_dcb_bias() = n; }
// from how many possible heads on the state machine takes its one-lane-per-unit form (the library: 8192)
void emu_ls2_fsm_lanes_min(int n) { ls2_fsm_lanes_min() = n; }

// gate_scan_kernel in streaming mode (mode 1) on one call's worth of samples.
// seek_type: -1 none, 0 SEEK_RN16, 1 SEEK_EPC applied before the scan (gate_impl.cc:112-123).
int emu_gate_stream(void *state_blob, const float *in, int n_in, int seek_type, float *out, int *consumed,
                    int *written, int *gate_open) {
  EmuRun run;
  GateState *st = reinterpret_cast<GateState *>(state_blob);
  if (seek_type >= 0) {
    st->n_samples = 0;
    st->wtype = seek_type;
    st->n_to_ungate = seek_type ? EPC_WIN : RN16_WIN;
  }
  int io[2] = {n_in, 0};
  if (n_in > 0) {
    GateArgs ga = {};
    ga.y = reinterpret_cast<const float2 *>(in); ga.y_stride = n_in; ga.n_dec = n_in; ga.lens = nullptr;
    ga.pos0 = 0; ga.chunk_len = n_in; ga.state = st; ga.n_streams = 1; ga.wtab = nullptr; ga.wmax = 0; ga.wcount = nullptr; ga.flat = nullptr;
    ga.flat_count = nullptr; ga.flat_cap = 0; ga.mode = 1; ga.gated = reinterpret_cast<float2 *>(out);
    ga.gated_cap = n_in; ga.io = io;
    emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{GATE_THREADS, 1, 1}, [&]() { gate_scan_kernel(ga); });
  }
  *consumed = io[0];
  *written = io[1];
  *gate_open = st->gate_open;
  return run.rc(0);
}

int emu_gate_state_size(void) { return (int)sizeof(GateState); }

// matched filter in streaming form (staging = 24 history samples + new samples)
int emu_mf_stream(const float *staging, int n_staging, int in_off, int n_out, float *out) {
  EmuRun run;
  if (n_out <= 0) return 0;
  std::vector<float4> ybuf((size_t)(n_out / 2 + 2));
  MfArgs ma;
  ma.x = reinterpret_cast<const float2 *>(staging); ma.x_stride = n_staging; ma.n_raw = n_staging; ma.lens = nullptr;
  ma.n_out = n_out; ma.in_off = in_off;
  ma.vec_ok = (in_off % 2 == 0 && (((uintptr_t)staging) & 15) == 0) ? 1 : 0;
  ma.y = reinterpret_cast<float2 *>(ybuf.data()); ma.y_stride = n_out; ma.tile0 = 0; ma.stream0 = 0;
  const int tiles = (n_out + MF_TILE - 1) / MF_TILE;
  emu::launch(emu::Idx3{(unsigned)tiles, 1, 1}, emu::Idx3{MF_THREADS, 1, 1}, [&]() { mf_boxcar25_decim5_kernel(ma); });
  memcpy(out, ybuf.data(), sizeof(float2) * (size_t)n_out);
  return run.rc(0);
}

// one window through decode_windows_kernel (input already DC-free, as the decoder block sees it)
int emu_decode_one(const float *win, int type, rfid_decode_result *res, rfid_scores *scores) {
  EmuRun run;
  const int wlen = type ? EPC_WIN : RN16_WIN;
  rfid_window w;
  w.stream = 0; w.seq = 0; w.start = 0; w.type = type; w.dc_re = 0.0f; w.dc_im = 0.0f;
  int one = 1;
  DecodeArgs da;
  da.y = reinterpret_cast<const float2 *>(win); da.y_stride = wlen; da.flat = &w; da.flat_count = &one;
  da.flat_cap = 1; da.res = res; da.scores = scores; da.wmax = 1;
  rfidh::t_candidates(da.t_cand, 400000);
  memset(scores, 0, sizeof(*scores));
  emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { decode_windows_kernel(da); });
  return run.rc(0);
}

// caller-given window lists through the batched decoders: which 0 = decode_all_kernel (as rfid_batch_decode launches it), 1 =
// decode_epc3_kernel alone, 2 = decode_rn16x4_kernel alone, on n_wg one-wave workgroups.  y: one row of n_y samples; the windows
// give start, dc and type themselves (stream 0, seq < wmax: the slot of res / scores / sum, which the caller prefills -- the
// slots of windows in no list must come back untouched).  A list of length 0 may be a null pointer.  tickets[2]: the launch's
// ticket counter and the next launch's, as decode_all_kernel leaves them (given in: 0 and a non-zero value).
int emu_decode_lists(const float *y, long n_y, const rfid_window *epc, int n_epc, const rfid_window *rn16, int n_rn16, int which,
                     int n_wg, int wmax, rfid_decode_result *res, rfid_scores *scores, int *sum, int *tickets) {
  EmuRun run;
  if (n_wg < 1 || n_epc < 0 || n_rn16 < 0 || (n_epc && !epc) || (n_rn16 && !rn16)) return -1;
  for (int k = 0; k < n_epc + n_rn16; ++k) {   // every window inside y and inside the result tables, and in the list of its type
    const rfid_window &w = (k < n_epc) ? epc[k] : rn16[k - n_epc];
    const int type = (k < n_epc) ? RFID_DECODE_EPC : RFID_DECODE_RN16;
    if (w.type != type || w.stream != 0 || w.seq < 0 || w.seq >= wmax || w.start < 0 ||
        (long)w.start + (type ? EPC_WIN : RN16_WIN) > n_y)
      return -1;
  }
  DecodeListArgs da;
  da.y = reinterpret_cast<const float2 *>(y); da.y_stride = n_y; da.cap = wmax; da.res = res; da.scores = scores; da.wmax = wmax;
  da.sum = sum;
  rfidh::t_candidates(da.t_cand, 400000);
  DecodeAllArgs all;
  all.epc = da; all.rn16 = da; all.ticket = &tickets[0]; all.ticket_next = &tickets[1];
  all.epc.list = epc; all.epc.count = &n_epc;
  all.rn16.list = rn16; all.rn16.count = &n_rn16;
  const emu::Idx3 grid{(unsigned)n_wg, 1, 1}, block{64, 1, 1};
  if (which == 0) emu::launch(grid, block, [&]() { decode_all_kernel(all); }, "decode_all_kernel");
  else if (which == 1) emu::launch(grid, block, [&]() { decode_epc3_kernel(all.epc); }, "decode_epc3_kernel");
  else if (which == 2) emu::launch(grid, block, [&]() { decode_rn16x4_kernel(all.rn16); }, "decode_rn16x4_kernel");
  else return -1;
  return run.rc(0);
}

// primitives self-test kernel
int emu_selftest(const float *x, const float *num, const float *den, float carry, float *chain_out,
                 float *div_out, float *hyp_out, float *shr_out) {
  EmuRun run;
  SelfTestArgs a;
  a.x = x; a.num = num; a.den = den; a.carry = carry; a.chain_out = chain_out; a.div_out = div_out;
  a.hyp_out = hyp_out; a.shr_out = shr_out; a.scan_out = nullptr;
  emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { selftest_kernel(a); });
  return run.rc(0);
}

// gate_fsm_step on caller-given records: gate_fsm_selftest_kernel as rfid_selftest_gate_fsm launches it
int emu_gate_fsm_selftest(const rfid_gate_fsm_in *in, int n, rfid_gate_fsm_out *out_wave, rfid_gate_fsm_out *out_lane) {
  EmuRun run;
  if (n <= 0) return 0;
  GateFsmSelfTestArgs a;
  a.in = in; a.out_wave = out_wave; a.out_lane = out_lane; a.n = n;
  emu::launch(emu::Idx3{(unsigned)((n + 63) / 64), 1, 1}, emu::Idx3{64, 1, 1}, [&]() { gate_fsm_selftest_kernel(a); });
  return run.rc(0);
}

// stream_stats_kernel on a caller-given result table, as rfid_selftest_stats launches it: `waves` wavefronts per trace, from the
// records or from their summaries (stats_summary_selftest_kernel; a fresh 256-byte aligned [n_streams * wmax + 4] array, as a
// plan's d_sum, the four words behind the table preset to reads of tag 255).  The kernel writes the caller's `out` itself.
// -2: the kernel issued a 16-byte load on an address that is no multiple of 16 (the device form reads an int4).
int emu_stats_selftest(const rfid_decode_result *res, const int *wcount, int n_streams, int wmax, int waves, int from_summaries,
                       int max_slot_number, int max_num_queries, int number_unique_tags, rfid_stream_stats *out) {
  EmuRun run;
  if (n_streams <= 0 || wmax <= 0 || waves < 1 || waves > STATS_MAX_WAVES || max_slot_number < 1) return -1;
  for (int s = 0; s < n_streams; ++s)
    if (wcount[s] < 0 || wcount[s] > wmax) return -1;
  const size_t n = (size_t)n_streams * (size_t)wmax;
  int *sum = nullptr;
  if (from_summaries) {
    void *p = nullptr;
    if (posix_memalign(&p, 256, sizeof(int) * (n + 4)) != 0) return -1;
    sum = (int *)p;
    memset(sum, 0xFF, sizeof(int) * (n + 4));
    StatsSummaryArgs ss;
    ss.res = res; ss.sum = sum; ss.n = (int64_t)n;
    emu::launch(emu::Idx3{(unsigned)((n + 255) / 256), 1, 1}, emu::Idx3{256, 1, 1}, [&]() { stats_summary_selftest_kernel(ss); });
  }
  StatsArgs sa;
  sa.res = res; sa.wcount = wcount; sa.wmax = wmax; sa.n_streams = n_streams;
  sa.max_slot_number = max_slot_number; sa.max_num_queries = max_num_queries; sa.number_unique_tags = number_unique_tags;
  sa.out = out; sa.sum = sum;
  emu::g_misaligned16 = 0;
  emu::launch(emu::Idx3{(unsigned)n_streams, 1, 1}, emu::Idx3{64 * (unsigned)waves, 1, 1}, [&]() { stream_stats_kernel(sa); });
  free(sum);
  return run.rc(emu::g_misaligned16 ? -2 : 0);      // (-2: a 16-byte load of the kernel was not 16-byte aligned)
}

// the inventory's and the tracks' kernels on a caller-given result table, as rfid_selftest_inventory launches them (launch_inventory /
// launch_tracks of csrc/rfid_capi.hip: the same five launches, the same choice of instantiation, restated here because that file is
// not part of this library).  The kernels write the caller's arrays themselves.  -1: an argument outside the entry's ranges; -2: a
// 16-byte load of a kernel on an address that is no multiple of 16.
int emu_inventory_selftest(const rfid_decode_result *res, const int *wcount, const int *n_windows_used, const int *start, int n_streams,
                           int wmax, int waves, int max_tags, int slots, long reads_cap, rfid_tag_entry *rows, int *counts, int *overflow,
                           int *head, int *ent_off, rfid_tag_entry *packed, int *base, int *reads_head, int64_t *offsets, rfid_tag_read *reads) {
  EmuRun run;
  if (n_streams <= 0 || wmax <= 0 || (waves != 1 && waves != INV_MAX_WAVES) || max_tags < 1 || max_tags > 512 || slots < 2 || slots > 1024 ||
      (slots & (slots - 1)) || reads_cap < 0)
    return -1;
  for (int s = 0; s < n_streams; ++s)
    if (wcount[s] < 0 || wcount[s] > wmax) return -1;
  const size_t n = (size_t)n_streams * (size_t)wmax;
  std::vector<rfid_window> wtab(n);
  std::vector<rfid_stream_stats> stats((size_t)n_streams);
  memset(stats.data(), 0, sizeof(rfid_stream_stats) * stats.size());
  for (int s = 0; s < n_streams; ++s) {
    stats[(size_t)s].n_windows = wcount[s];
    stats[(size_t)s].n_windows_used = n_windows_used[s];
    for (int k = 0; k < wmax; ++k) {
      rfid_window &w = wtab[(size_t)s * (size_t)wmax + (size_t)k];
      w.stream = s; w.seq = k; w.start = start[(size_t)s * (size_t)wmax + (size_t)k]; w.type = k & 1; w.dc_re = 0.0f; w.dc_im = 0.0f;
    }
  }
  InvArgs a;
  a.res = res; a.wcount = wcount; a.stats = stats.data(); a.wmax = wmax; a.n_streams = n_streams;
  a.max_tags = max_tags; a.slots = slots; a.out = rows; a.counts = counts; a.overflow = overflow;
  InvPackArgs p;
  p.in = rows; p.counts = counts; p.overflow = overflow; p.n_streams = n_streams; p.max_tags = max_tags;
  p.offsets = ent_off; p.head = head; p.packed = packed;
  TrkScanArgs sp;
  sp.ent = rows; sp.counts = counts; sp.inv_head = head; sp.n_streams = n_streams; sp.max_tags = max_tags;
  sp.base = base; sp.head = reads_head; sp.offsets = offsets;
  TrkArgs t;
  t.res = res; t.wtab = wtab.data(); t.wcount = wcount; t.stats = stats.data(); t.wmax = wmax; t.n_streams = n_streams;
  t.ent = rows; t.counts = counts; t.ent_off = ent_off; t.max_tags = max_tags; t.slots = slots;
  t.base = base; t.out = reads; t.cap = reads_cap; t.offsets = offsets;
  const emu::Idx3 grid{(unsigned)n_streams, 1, 1}, block{64 * (unsigned)waves, 1, 1};
  const emu::Idx3 one{1, 1, 1}, scan{(unsigned)((n_streams >= INV_SCAN_THREADS) ? INV_SCAN_THREADS : ((n_streams + 63) & ~63)), 1, 1};
  emu::g_misaligned16 = 0;
  if (slots <= 128) emu::launch(grid, block, [&]() { inventory_kernel<128>(a); }, "inventory_kernel<128>");
  else emu::launch(grid, block, [&]() { inventory_kernel<1024>(a); }, "inventory_kernel<1024>");
  emu::launch(one, scan, [&]() { inventory_offsets_kernel(p); }, "inventory_offsets_kernel");
  emu::launch(grid, emu::Idx3{64, 1, 1}, [&]() { inventory_pack_kernel(p); }, "inventory_pack_kernel");
  emu::launch(one, scan, [&]() { tracks_offsets_kernel(sp); }, "tracks_offsets_kernel");
  const bool small = slots <= 128 && max_tags <= 64, wide = waves > 1;
  if (small && !wide) emu::launch(grid, block, [&]() { tracks_kernel<128, 64, 1>(t); }, "tracks_kernel<128, 64, 1>");
  else if (!wide) emu::launch(grid, block, [&]() { tracks_kernel<1024, 512, 1>(t); }, "tracks_kernel<1024, 512, 1>");
  else if (small) emu::launch(grid, block, [&]() { tracks_kernel<128, 64, INV_MAX_WAVES>(t); }, "tracks_kernel<128, 64, 16>");
  else emu::launch(grid, block, [&]() { tracks_kernel<1024, 512, INV_MAX_WAVES>(t); }, "tracks_kernel<1024, 512, 16>");
  return run.rc(emu::g_misaligned16 ? -2 : 0);
}

// in-order sum: the integer-scan form against the chain; scan_out[64] = 1 when the scan was provably exact
int emu_chain_scan(const float *x, float carry, float *chain_out, float *scan_out) {
  EmuRun run;
  std::vector<float> z(64, 1.0f), o(64 * 3);
  SelfTestArgs a;
  a.x = x; a.num = z.data(); a.den = z.data(); a.carry = carry; a.chain_out = chain_out; a.div_out = o.data();
  a.hyp_out = o.data() + 64; a.shr_out = o.data() + 128; a.scan_out = scan_out;
  emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{64, 1, 1}, [&]() { selftest_kernel(a); });
  return run.rc(0);
}

// chain_add_auto2 (long-stream front end: the in-order sums from two carries at once) on one step; scanned[0] = 1 when the
// shared integer-scan form applied
int emu_chain_scan2(const float *x, float ca, float cb, float *out_a, float *out_b, int *scanned) {
  EmuRun run;
  struct Args { const float *x; float ca, cb; float *oa, *ob; int *sc; } a = {x, ca, cb, out_a, out_b, scanned};
  emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{64, 1, 1}, [&]() {
    const int lane = wv::lane_id();
    float va, vb;
    const bool ok = chain_add_scan2(a.ca, a.cb, a.x[lane], lane, va, vb);
    if (lane == 0) a.sc[0] = ok ? 1 : 0;
    chain_add_auto2(a.ca, a.cb, a.x[lane], lane, va, vb);
    a.oa[lane] = va; a.ob[lane] = vb;
  });
  return run.rc(0);
}

// synthetic-replica generator (workload generator, not on the receive path)
int emu_synth_replicas(const float *base, long n_raw, float *out, long out_stride, int n_streams, float sigma,
                       unsigned long long seed, long first_replica) {
  EmuRun run;
  if (n_raw <= 0 || n_streams <= 0) return 0;
  SynthArgs a;
  a.base = reinterpret_cast<const float2 *>(base); a.out = reinterpret_cast<float2 *>(out); a.n_raw = n_raw;
  a.out_stride = out_stride; a.first_replica = first_replica; a.sigma = sigma;
  a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32);
  const long per_block = (long)SYNTH_THREADS * SYNTH_PAIRS_PER_THREAD * 2;
  const long blocks = (n_raw + per_block - 1) / per_block;
  emu::launch(emu::Idx3{(unsigned)blocks, (unsigned)n_streams, 1}, emu::Idx3{SYNTH_THREADS, 1, 1},
              [&]() { synth_replicas_kernel(a); });
  return run.rc(0);
}

// Gen2 trace synthesiser (workload generator): the same host layout as rfid_synth_gen2, the kernel emulated
long emu_synth_gen2(const rfid_synth_gen2_params *p, const rfid_synth_slot *slots, long n_slots, float *out, long out_cap,
                    float sigma, unsigned long long seed, long replica) {
  EmuRun run;
  std::vector<Gen2SlotDev> dev;
  const int64_t total = rfidh::gen2_layout(*p, slots, n_slots, &dev);
  if (total < 0 || total > out_cap) return -1;
  Gen2Args a;
  memset(&a, 0, sizeof(a));
  a.slots = dev.data(); a.n_slots = (int64_t)dev.size(); a.out = reinterpret_cast<float2 *>(out); a.n_raw = total;
  a.leak_re = p->leak_re; a.leak_im = p->leak_im;
  for (int k = 0; k < G2_MAX_TAGS; ++k) { a.h_re[k] = p->h_re[k]; a.h_im[k] = p->h_im[k]; }
  a.sigma = sigma; a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.replica = (uint64_t)replica;
  emu::launch(emu::Idx3{(unsigned)dev.size(), 1, 1}, emu::Idx3{G2_THREADS, 1, 1}, [&]() { synth_gen2_kernel(a); });
  return run.rc(0) ? (long)EMU_DEADLOCK : (long)total;
}

void emu_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  uint32_t o[4];
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
  for (int i = 0; i < 4; ++i) out[i] = o[i];
}

}  // extern "C"
