"""Builds tests/wave_emu/librfid_wave_emu.so and librfid_wave_emu_wpb1.so (TEST INFRASTRUCTURE: host emulation of the
kernels for the GPU-less CI container; never part of the product)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "gen2-uhf-rfid-reader_amd", "csrc")
OUT = os.path.join(HERE, "librfid_wave_emu.so")
# waves per workgroup of the dc_est finishing walk (LS2_FIN_WPB): 16 (the default) and 1, the device's (one-wave workgroups that meet)
VARIANTS = {16: OUT, 1: os.path.join(HERE, "librfid_wave_emu_wpb1.so")}


def build(force: bool = False, fin_wpb: int = 16) -> str:
    out = VARIANTS[fin_wpb]
    srcs = [os.path.join(HERE, "emu_driver.cpp"), os.path.join(HERE, "rfid_device_env.h"),
            os.path.join(CSRC, "rfid_kernels.hpp"), os.path.join(CSRC, "rfid_ls2.hpp"), os.path.join(CSRC, "rfid_ls2_enqueue.hpp"),
            os.path.join(CSRC, "rfid_stage.hpp"), os.path.join(CSRC, "rfid_inventory.hpp"), os.path.join(CSRC, "rfid_tracks.hpp"),
            os.path.join(CSRC, "rfid_host_math.h"),
            os.path.join(CSRC, "rfid_gen2_host.h"),
            os.path.join(ROOT, "include", "rfid_mi355x.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(s) <= os.path.getmtime(out) for s in srcs + [__file__]):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-fno-strict-aliasing",
           "-DLS2_FIN_WPB=%d" % fin_wpb,
           "-I", HERE,                       # the emulator's rfid_device_env.h shadows the HIP one
           "-I", os.path.join(ROOT, "include"), "-iquote", HERE,
           "-o", out + ".tmp", os.path.join(HERE, "emu_driver.cpp"), "-I", CSRC]
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    for w in VARIANTS:
        print(build(force=True, fin_wpb=w))
