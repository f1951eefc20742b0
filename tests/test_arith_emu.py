"""The arithmetic primitives on the crafted operands of tests/arith_cases.py, on the emulator (tests/test_gpu_arith.py: the same
bodies on the device).  First the reference alone: tests/arith_ref.py pinned to exact rational arithmetic, and what every family
reaches asserted from it -- no kernel has run by then.  Then rfid_selftest_arith through the stand-in runtime.

What that run can show differs by primitive.  The in-order sums, their scan shortcuts and flags, and the constant divisions with
their admission votes are the product's source on both sides: a mismatch here is a mismatch there.  hypot_f, lds_sum25_in_order,
scan_add, the DPP building blocks, fdiv, rint_f and shr1 are the emulator's own restatements (tests/wave_emu/rfid_device_env.h):
for those this module checks the cases, the reference and that restatement, and only the device module says anything about the
device forms (the rsq + Newton sequence, the ds_read batches, the DPP controls, __fdiv_rn, v_rndne)."""
import pytest

import arith_cases as ac
import arith_suite as suite


@pytest.fixture(scope="module")
def built():
    cases, pairs = ac.build()
    return cases, pairs, suite.facts_of(cases)


@pytest.fixture(scope="module")
def capi_ctx():
    import emu_lib
    with emu_lib.emulated_library():
        import rfid
        c = rfid.Context(device=0)
        try:
            yield c
        finally:
            c.close()


# ---- the reference and the cases, no kernel ------------------------------------------------------------------------------------
def test_reference_additions_and_rounding_are_exact(built):
    suite.check_additions_pinned(built[0])
    suite.check_rint_pinned(built[0])


def test_sum_families_reach_what_they_are_named_for(built):
    suite.check_sum_reach(built[0], built[2])


def test_division_families_and_the_exact_quotient(built):
    suite.check_division_reach(built[0])


def test_hypot_families_and_the_exact_formula(built):
    suite.check_hypot_reach(built[1])


def test_tile_and_scan_families(built):
    suite.check_tile_reach(built[0])
    suite.check_scan_reach(built[0])


# ---- the kernels on the emulator -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ac.GROUPS)
def test_primitives_on_crafted_operands(capi_ctx, built, group):
    cases, _, facts = built
    suite.run(capi_ctx, cases, facts, group)
