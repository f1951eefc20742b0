"""The arithmetic primitives in their device forms on the crafted operands of tests/arith_cases.py (tests/test_arith_emu.py: the
same bodies on the emulator, and the reach of every family).  The device run is the only evidence for what the emulator
restates: hypot_f's v_rsq_f64 + Newton sequence, the ds_read batches and waits of lds_sum25_in_order, the DPP controls of
scan_add / shr1 / the building blocks, __fdiv_rn and v_rndne."""
import pytest

import arith_cases as ac
import arith_suite as suite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    cases, pairs = ac.build()
    return cases, pairs, suite.facts_of(cases)


def test_reference_agrees_with_itself_here(built):
    """the exact-integer hypot formula against numpy's on this machine, before the device is believed against either"""
    suite.check_hypot_reach(built[1])


@pytest.mark.parametrize("group", ac.GROUPS)
def test_primitives_on_crafted_operands(gpu_ctx, built, group):
    cases, _, facts = built
    suite.run(gpu_ctx, cases, facts, group)
