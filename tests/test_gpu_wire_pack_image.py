"""The whole descriptor's pack stage alone (wire_pack_image_kernel in csrc/wire_pack.hip through omni_wire_pack_image_enqueue_dev) against the g++ build of the layout
it runs (csrc/wire_plan.h inside omni_wire_pack_image_host, which tests/test_wire_image_plan_cpu.py holds to LoopNetWire byte for byte): sizes and buffers identical,
every byte -- the bytes behind a packet's last dword included, which neither side may write (both start from 0xA5).  Shapes (tests/wire_image_cases.py): n_images 1 and
8, max_num 65 and 200, n_kps 0 / 1 / 2 / 3 / 4 / 65 / 200 and clamped counts (every alignment of the byte tail), file sizes of every residue mod 4 against each of
them, no file (status TRUNCATED), the smallest file, exactly the capacity, above it (clamped), all four (with_features, with_image) combinations, NaN / inf / -0.0
payload bits; and what is refused before any launch."""
import numpy as np
import pytest

from omni_swarm_amd import capi
from tests import wire_image_cases as IC

CASES = IC.cases(capi)


@pytest.fixture(scope="module")
def host_packed():
    """name -> (packets, sizes) of the g++ build; computed once"""
    return {name: capi.wire_pack_image_host(*IC.args(f), **IC.kwargs(f), fill=0xA5) for name, f in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_host_function(ctx, host_packed, name):
    f = CASES[name]
    out, sizes = capi.wire_pack_image(ctx, *IC.args(f), **IC.kwargs(f), fill=0xA5)
    want_out, want_sizes = host_packed[name]
    print(f"{name}: packet sizes {sizes[:, 1].tolist()}, differing bytes {int((out != want_out).sum())}, differing size entries {int((sizes != want_sizes).sum())}")
    assert np.array_equal(sizes, want_sizes)
    assert np.array_equal(out, want_out)
    for g in range(len(sizes)):                              # (stated here too: nothing behind the packet's last dword, whatever the host function does)
        assert np.all(out[g, (sizes[g, 0] + sizes[g, 1] + 3) // 4 * 4 if sizes[g, 1] else 0:] == 0xA5)


@pytest.mark.gpu
def test_refused_before_any_launch(ctx):
    f = CASES["random_1x65_f1i1"]
    ins = [a.view(np.uint8) if a.dtype == capi.WIRE_META_DTYPE else a for a in IC.args(f)]
    dev = [ctx.to_device(a) for a in ins]
    out, sizes = ctx.alloc(capi.wire_image_capacity(65, 1024) + 4), ctx.alloc(8)
    call = lambda n_images=1, max_num=65, jp=dev[8:], cap=1024, o=out, **kw: capi.wire_pack_image_dev(ctx, n_images, max_num, *dev[:8], *jp, cap, 640, 480, o, sizes, **kw)
    try:
        for kw, word in (({"desc_dim": 256}, "64"), ({"global_dim": 1024}, "4096"), ({"n_images": 0}, "n_images"), ({"max_num": 0}, "max_num"), ({"max_num": 1025}, "max_num"),
                         ({"cap": 1022}, "multiple of 4"), ({"cap": -4}, "jpeg_capacity"), ({"cap": 2**30 + 4}, "jpeg_capacity"), ({"with_image": False}, "null exactly"),
                         ({"jp": [None] * 3}, "null exactly"), ({"jp": [dev[8], dev[9], None]}, "null exactly"), ({"o": out + 2}, "aligned"),
                         ({"jp": [dev[8] + 2, dev[9], dev[10]]}, "aligned")):
            with pytest.raises(capi.OmniError, match=word):
                call(**kw)
        with pytest.raises(capi.OmniError, match="null"):
            capi.wire_pack_image_dev(ctx, 1, 65, *dev[:7], None, *dev[8:], 1024, 640, 480, out, sizes)
        call(jp=[None] * 3, cap=0, with_image=False)          # (the three pointers null with with_image 0: accepted)
        ctx.sync()
    finally:
        for p in dev + [out, sizes]:
            ctx.free(p)
