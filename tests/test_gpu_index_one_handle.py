"""GPU: ONE fp32 index handle through every owner of its rows and every path of a search (csrc/index_plan.h) -- row-by-row growth that carries the fp16 mirror
over, a batch through the mirror + certificate, the same queries below the matrix-core threshold on the exact scan, a snapshot loaded into a second handle, and
the first handle again after omni_index_set_shard dropped its mirror.  Scores and ids of all of them are the same bits: that is what the certificate promises."""
import os

import numpy as np
import pytest

from oracle import match_ref as M
from tests.test_gpu_index import _check

pytestmark = pytest.mark.gpu
DIM, N, NQ, K = 512, 1030, 9, 5


def test_one_handle_grows_searches_on_every_path_saves_loads_and_drops_its_mirror(omni, ctx, tmp_path):
    assert os.environ.get("OMNI_INDEX_MIRROR_MIN_ROWS") == "0"               # the suite's setting: small databases go through the mirror
    rng = np.random.default_rng(1030)
    db = rng.standard_normal((N, DIM)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    q = db[[0, 511, 1023, 1024, 1029, 7, 300, 1000, 1025]] + 0.05 * rng.standard_normal((NQ, DIM)).astype(np.float32)
    idx = omni.capi.IndexFlatIP(ctx, DIM, omni.capi.STORE_F32, 0)
    for row in db:                                                           # 1024 -> 2048 rows with a mirror to carry over
        idx.add(row)
    assert idx.ntotal == N
    # a batch: through the mirror
    s0, f0 = idx.cert_stats()
    D, I = idx.search(q, K)
    s1, f1 = idx.cert_stats()
    assert s1 - s0 == NQ
    _check(idx, db, q, K)
    Dr, Ir = M.ip_search(db, q, K)
    assert np.array_equal(I, Ir)
    s1, f1 = idx.cert_stats()
    # below the matrix-core threshold: the exact scan, the same bits
    D3, I3 = idx.search(q[:3], K)
    assert idx.cert_stats() == (s1, f1)
    assert np.array_equal(I3, I[:3]) and np.array_equal(D3, D[:3])
    # a snapshot in a second handle
    path = str(tmp_path / "one_handle.omnx")
    idx.save(path)
    idx2 = omni.capi.IndexFlatIP(ctx, DIM, omni.capi.STORE_F32, 0)
    idx2.load(path)
    assert idx2.ntotal == N
    D2, I2 = idx2.search(q, K)
    assert idx2.cert_stats()[0] == NQ                                         # its mirror was rebuilt from the loaded rows
    assert np.array_equal(I2, I) and np.array_equal(D2, D)
    # sharded: no mirror, no certificate, the same bits
    idx.set_shard(0, 1)
    Ds, Is = idx.search(q, K)
    assert idx.cert_stats() == (s1, f1)
    assert np.array_equal(Is, I) and np.array_equal(Ds, D)
    idx2.close()
    idx.close()
