"""The LoopNet wire's pack stage alone (csrc/wire_pack.hip through omni_wire_pack_enqueue_dev) against the g++ build of the layout it runs (csrc/wire_plan.h inside
omni_wire_pack_host, which tests/test_wire_plan_cpu.py holds to LoopNetWire byte for byte): tables and buffers identical, every byte -- the bytes behind an image's
last packet included, which neither side may write (both start from 0xA5).  Shapes: n_images 1 and 8, max_num 200 and 65, 600 and 1024 (more than one compaction
pass), and the edges: no key points, no flag, all flagged, 63 / 64 / 65 flagged of 200, send_all_features, clamped counts, NaN / inf / -0.0 bits."""
import numpy as np
import pytest

from omni_swarm_amd import capi
from tests import wire_cases as WC

CASES = WC.cases(capi)


@pytest.fixture(scope="module")
def host_packed():
    """name -> (packets, table) of the g++ build; computed once"""
    return {name: capi.wire_pack_host(*WC.args(f), send_all_features=f["send_all_features"], fill=0xA5) for name, f in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_host_function(ctx, host_packed, name):
    f = CASES[name]
    out, table = capi.wire_pack(ctx, *WC.args(f), send_all_features=f["send_all_features"], fill=0xA5)
    want_out, want_table = host_packed[name]
    print(f"{name}: packets per image {table[:, 0].tolist()}, bytes used {table[:, 1].tolist()}, differing bytes {int((out != want_out).sum())}, "
          f"differing table entries {int((table != want_table).sum())}")
    assert np.array_equal(table, want_table)
    assert np.array_equal(out, want_out)


@pytest.mark.gpu
def test_refused_before_any_launch(ctx):
    f = CASES["random_1x65"]
    dev = [ctx.to_device(a.view(np.uint8) if a.dtype == capi.WIRE_META_DTYPE else a) for a in WC.args(f)]
    out, table = ctx.alloc(capi.wire_packet_capacity(65) + 4), ctx.alloc(4 * capi.wire_table_ints(65))
    try:
        for kw, word in (({"desc_dim": 256}, "64"), ({"global_dim": 1024}, "4096")):
            with pytest.raises(capi.OmniError, match=word):
                capi.wire_pack_dev(ctx, 1, 65, *dev, out, table, **kw)
        for n_images, max_num, word in ((1, 0, "max_num"), (1, 1025, "max_num"), (0, 65, "n_images")):
            with pytest.raises(capi.OmniError, match=word):
                capi.wire_pack_dev(ctx, n_images, max_num, *dev, out, table)
        with pytest.raises(capi.OmniError, match="aligned"):
            capi.wire_pack_dev(ctx, 1, 65, *dev, out + 2, table)
        with pytest.raises(capi.OmniError, match="null"):
            capi.wire_pack_dev(ctx, 1, 65, *dev[:-1], None, out, table)
        ctx.sync()
    finally:
        for p in dev + [out, table]:
            ctx.free(p)
