// tests/wave_emu/emu_front_pairs.cpp -- TEST INFRASTRUCTURE ONLY: the emulator driver plus entry points for the helpers of
// front_end_fused_kernel's pair body that no batch output shows bit for bit (avg_ampl only feeds threshold votes).  Built by
// tests/test_emu_front_pairs.py into a temporary directory.
#include "emu_driver.cpp"

extern "C" {

// chain_add_scan_pair on two steps from one carry: out0 / out1 = its sums, ok[0] = 1 when it declares them exact;
// ref0 / ref1 = the 63-step chain (chain_add) step after step
int emu_chain_scan_pair(const float *x0, const float *x1, float carry, float *out0, float *out1, float *ref0, float *ref1, int *ok) {
  EmuRun run;
  emu::launch(emu::Idx3{1, 1, 1}, emu::Idx3{64, 1, 1}, [&]() {
    const int lane = wv::lane_id();
    float v0, v1;
    const bool good = chain_add_scan_pair(carry, x0[lane], x1[lane], lane, v0, v1);
    if (lane == 0) ok[0] = good ? 1 : 0;
    out0[lane] = v0; out1[lane] = v1;
    const float r0 = chain_add(carry, x0[lane], lane);
    const float r1 = chain_add(wv::readlane(r0, 63), x1[lane], lane);
    ref0[lane] = r0; ref1[lane] = r1;
  });
  return run.rc(0);
}

}  // extern "C"
