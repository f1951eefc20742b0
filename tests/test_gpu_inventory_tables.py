"""inventory_kernel, inventory_offsets_kernel, inventory_pack_kernel, tracks_offsets_kernel and tracks_kernel by themselves on the
crafted and the random result tables of tests/inventory_cases.py, on the device (tests/test_inventory_tables_emu.py: the same on
the emulator, with the pinning of the reference and the coverage conditions).  Every table through rfid_selftest_inventory -- the
product's launch sequence and its choice of instantiation -- in the product's two workgroup shapes, one wave and sixteen per trace;
every word of every output array against tests/inventory_ref.py and tests/tracks_ref.py, the words the kernels have no business
writing included."""
import pytest

import inventory_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rfid
    c = rfid.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def launches():
    by = {}
    for g in ic.launches():
        by.setdefault(g.family, []).append(g)
    return by


def test_every_table_is_launched(launches):
    names = [n for gs in launches.values() for g in gs for n in g.names]
    assert len(names) == len(set(names)) >= 290 and set(launches) == set(ic.FAMILIES)
    assert {"nw%d" % n for n in ic.NW_LIST} <= set(names) and len([n for n in names if n.startswith("random")]) == ic.N_RANDOM
    assert {len(g.res) for g in launches["batches"]} == set(ic.BATCH_SIZES)


@pytest.mark.parametrize("family", ic.FAMILIES)
@pytest.mark.parametrize("waves", ic.WAVES)
def test_kernels_on_the_device(ctx, launches, waves, family):
    for g in launches[family]:
        ic.check(ctx.selftest_inventory, g, waves)
