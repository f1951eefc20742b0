// tests/tools/host_pass_check.cpp -- TEST INFRASTRUCTURE: the host side of a batch pass under the host sanitizers.  A program of
// its own that links csrc/rfid_capi.hip compiled against tests/fake_hip (the kernels run on the wave emulator): two traces made by the
// library's own synthesiser, then two passes each through the fused front end (mode 0) and the long-stream front end (mode 2) with the
// four stages behind them.  Not part of the suite; from the repository root:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fno-strict-aliasing -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -DLS2_FIN_WPB=16 -I tests/fake_hip -I tests/wave_emu -I include -iquote tests/wave_emu -I gen2-uhf-rfid-reader_amd/csrc \
//       -x c++ gen2-uhf-rfid-reader_amd/csrc/rfid_capi.hip tests/wave_emu/emu_driver.cpp tests/tools/host_pass_check.cpp -o host_pass_check
//   ./host_pass_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include "rfid_mi355x.h"

#define OK(call) do { const int rc__ = (call); if (rc__ != RFID_OK) { fprintf(stderr, "%s -> %d (%s)\n", #call, rc__, rfid_last_error(c)); return 1; } } while (0)

int main() {
  rfid_params prm;
  rfid_params_default(&prm);
  rfid_ctx *c = nullptr;
  OK(rfid_ctx_create(&prm, 0, &c));
  // one tag answering in every slot (the EPC frames are arbitrary bits: their CRC fails, which is what the repair stage looks at)
  const int n_slots = 6, B = 2;
  rfid_synth_gen2_params p;
  memset(&p, 0, sizeof(p));
  p.leak_re = 0.7648f; p.leak_im = 0.6442f; p.h_re[0] = 0.06f; p.h_im[0] = 0.03f; p.n_tags = 1; p.tail_us = 200;
  std::vector<rfid_synth_slot> slots((size_t)n_slots);
  for (int i = 0; i < n_slots; ++i) {
    rfid_synth_slot &s = slots[(size_t)i];
    memset(&s, 0, sizeof(s));
    s.cmd = (i == 0) ? 0 : 1; s.n_tags = 1; s.has_epc = 1;
    s.rn16[0] = (uint16_t)(0x5a5a ^ (i * 2654435761u)); s.ack = s.rn16[0];
    s.rn16_off_raw = 500; s.epc_off_raw = 500;
    for (int k = 0; k < 4; ++k) s.epc[k] = 0x3000f00fu * (uint32_t)(i + k + 1);
  }
  int64_t L = 0, n = 0;
  OK(rfid_synth_gen2_size(&p, slots.data(), n_slots, &L));
  const int64_t stride = (L + 1) & ~1LL;
  void *d_base = nullptr, *d_many = nullptr;
  if (hipMalloc(&d_base, sizeof(rfid_cf32) * (size_t)stride) != hipSuccess || hipMalloc(&d_many, sizeof(rfid_cf32) * (size_t)stride * B) != hipSuccess) return 1;
  OK(rfid_synth_gen2(c, &p, slots.data(), n_slots, d_base, stride, 0.0f, 77u, 0, &n));
  OK(rfid_synth_replicas(c, d_base, L, d_many, stride, B, 0.003f, 78u, 0));
  for (int mode = 0; mode <= 2; mode += 2) {
    OK(rfid_ctx_set_knob(c, "long_stream", mode));
    OK(rfid_batch_plan(c, B, L));
    OK(rfid_batch_plan_inventory(c, 8));
    OK(rfid_batch_plan_tracks(c));
    OK(rfid_batch_plan_quality(c));
    OK(rfid_batch_plan_repair(c));
    for (int pass = 0; pass < 2; ++pass) {
      OK(rfid_batch_process(c, d_many, stride, L, nullptr, 0));
      OK(rfid_batch_inventory(c));
      OK(rfid_batch_tracks(c));
      OK(rfid_batch_quality(c));
      OK(rfid_batch_repair(c));
    }
    OK(rfid_batch_sync(c));
    rfid_stream_stats st[B];
    OK(rfid_batch_get_stats(c, st, B));
    std::vector<rfid_read_quality> q((size_t)n_slots + 4);
    std::vector<rfid_repair> r((size_t)n_slots + 4);
    int64_t nq = 0, nr = 0;
    OK(rfid_batch_get_window_quality(c, 1, q.data(), (int64_t)q.size(), &nq));
    OK(rfid_batch_get_window_repairs(c, 1, r.data(), (int64_t)r.size(), &nr));
    rfid_batch_timing t;
    OK(rfid_batch_timing_get(c, &t));
    printf("mode %d: fused_front %d, windows %d + %d, EPC rows of trace 1: %lld / %lld\n", mode, t.fused_front, (int)st[0].n_windows, (int)st[1].n_windows,
           (long long)nq, (long long)nr);
    if (t.fused_front != (mode ? 2 : 1) || st[0].n_windows != 2 * n_slots || nq != n_slots || nr != n_slots) { fprintf(stderr, "unexpected\n"); return 1; }
  }
  (void)hipFree(d_base);
  (void)hipFree(d_many);
  OK(rfid_ctx_destroy(c));
  printf("ok\n");
  return 0;
}
