"""A lane of the key-frame pipeline makes MobileNetVLAD's own stream only when it is used: under OMNI_PIPELINE_ONE_STREAM=1 (MobileNetVLAD behind
SuperPoint on the lane's one stream) it creates none -- an idle stream would still take a hardware-queue slot (csrc/stream_plan.h).  The toy pipeline of
smoke() -- 5 key frames as 2 + 2 + a partial unit (a tail lane), then 4 of them again -- must return the same loop candidates, hits and database rows on
one stream per lane as on two, and sync()/close() must work without the second context."""
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def run_toy(omni, ctx, files, db, blocks):
    from omni_swarm_amd import pipeline
    c = omni.capi
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], 128, 96, 0.015, 100, c.PREC_F16, 2, 2, c.STORE_F32,
                                   1, 0.3, 0.2, 5, 10, 3)
    pl.preload(db[:40])
    ptrs = [blocks[0].ctypes.data, blocks[1].ctypes.data]
    hits = [pl.run(5, 0, ptrs, 0, blocks[2].ctypes.data, True), pl.run(4, 5, ptrs, 0, None, True)]
    pl.sync()
    out = (hits, int(pl.db_rows), pl.candidates().copy())
    pl.close()
    return out


def test_one_stream_lanes_return_what_two_stream_lanes_return(omni, ctx, monkeypatch):
    from omni_swarm_amd import synth, weights as W_
    from oracle import mobilenetvlad_ref, superpoint_ref
    comp, mean = synth.pca()
    db = synth.global_db(64, seed=3)
    blocks = []
    for p in range(3):
        mb = 2 if p < 2 else 1
        a = ctx.host_alloc((8 * mb, 96, 128), np.uint8)
        kf = [[synth.image_u8(900 + 8 * (2 * p + m) + i, 96, 128, n_shapes=60) for i in range(8)] for m in range(mb)]
        a[:] = np.stack([kf[m][i] for m in range(mb) for i in range(4)] + [kf[m][4 + i] for m in range(mb) for i in range(4)])
        blocks.append(a)
    with tempfile.TemporaryDirectory() as td:
        files = W_.write_pipeline_files(td, superpoint_ref.synth_weights(0), comp, mean, mobilenetvlad_ref.synth_weights(), mobilenetvlad_ref.layer_specs(),
                                        omni.capi.VLAD_KINDS)
        monkeypatch.delenv("OMNI_PIPELINE_ONE_STREAM", raising=False)
        two = run_toy(omni, ctx, files, db, blocks)
        monkeypatch.setenv("OMNI_PIPELINE_ONE_STREAM", "1")
        one = run_toy(omni, ctx, files, db, blocks)
    for a in blocks:
        ctx.host_free(a)
    assert two[0][1] == 4, two[0]                                      # the second visit of the same key frames closes a candidate each (smoke())
    assert two[1] == 40 + 9 * 4
    assert one[0] == two[0] and one[1] == two[1] and np.array_equal(one[2], two[2])
