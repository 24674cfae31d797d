"""CPU checks of the plan of an index search (csrc/index_plan.h, compiled with g++ under -fsanitize=address,undefined into tests/cpp/index_plan_pin.cpp): which
path a search takes, its candidate count and buffer sizes, its scan passes and their launches, for every combination of storage, mirror, dimension, queries, k,
rows and the three switches -- restated here independently, in the terms index.hip's search_dev / launch_scan / launch_scan_mq / ensure_capacity used before the
plan existed (the mirror condition, mq, max_qb, kp, per_q, the three grid rules, the capacity rule), and compared field by field; the rows the production
defaults take for the benchmark's shapes, by name; and that the host code of index.hip decides nothing next to the plan (no storage expression in search_dev, no
literal size, one owner of the rows)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omni-swarm_amd", "csrc")
F32, F16 = 0, 1                                                     # include/omni_hip.h OMNI_STORE_*
MIRROR_CERT, MQ_F16, EXACT_SCAN = 0, 1, 2                           # IndexSearchPath
ONE, ROWS, T16, MQ = 0, 1, 2, 3                                     # IndexScanForm
DIMS = [512, 1024, 4096, 8192]
NQS = [1, 2, 3, 4, 5, 7, 8, 9, 17, 33, 64, 65, 130, 4096]
KS = [1, 5, 32, 33, 40, 64, 65, 1024]
NS = [0, 1, 15, 16, 17, 2047, 2048, 2049, 32767, 32768, 100000, 125000, 400000]
MQ_MINS = [0, 1, 4]                                                 # OMNI_MQ_MIN: never, always, the default
ROWS_MINS = [4, 5, 9]                                               # OMNI_SCAN_ROWS_MIN: the default, 5, 9
MIRROR_MINS = [0, 32768]                                            # OMNI_INDEX_MIRROR_MIN_ROWS: the suite's, the default
CUS = [8, 256]
ROW = np.dtype([(n, np.int64) for n in ("per_q", "keys_bytes", "cert_keys_bytes", "n", "mirror_min", "sum_q0")] +
               [(n, np.int32) for n in ("storage", "mirror", "dim", "nq", "k", "mq_min", "rows_min", "n_cu", "path", "kp", "cert_flags_bytes", "hflags_bytes", "count",
                                        "width", "mq", "sum_qb", "n_one", "n_rows", "n_t16", "n_mq", "first_form", "first_grid", "last_q0", "last_qb", "last_form",
                                        "last_grid", "last_threads", "last_smem")])
INPUTS = ["storage", "mirror", "dim", "nq", "k", "n", "mq_min", "rows_min", "mirror_min", "n_cu"]


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("index_plan") / "index_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "index_plan_pin.cpp")])
    return exe


def text(pin, mode):
    return [line.split() for line in subprocess.run([pin, mode], capture_output=True, check=True, text=True).stdout.splitlines()]


@pytest.fixture(scope="module")
def rows(pin, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("index_plan_rows") / "plans.bin")
    subprocess.run([pin, "plans", out], check=True)
    t = np.fromfile(out, ROW)
    os.remove(out)
    lists = [[F32, F16], [0, 1], DIMS, NQS, KS, NS, MQ_MINS, ROWS_MINS, MIRROR_MINS, CUS]
    assert len(t) == np.prod([len(v) for v in lists])
    shape = [len(v) for v in lists]
    for i, (name, vals) in enumerate(zip(INPUTS, lists)):              # the rows are the full product, INPUTS[0] slowest
        want = np.broadcast_to(np.asarray(vals).reshape([-1 if j == i else 1 for j in range(len(shape))]), shape).ravel()
        assert np.array_equal(t[name], want), name
    return {n: t[n].astype(np.int64) for n in ROW.names}


def cdiv(a, b):
    return (a + b - 1) // b


def parent_query_block(dim):
    """search_dev: int max_qb = 131072 / (dim * 4); max_qb = max_qb > SCAN_MAX_QB ? SCAN_MAX_QB : (max_qb < 1 ? 1 : max_qb)"""
    max_qb = 131072 // (dim * 4)
    return np.where(max_qb > 8, 8, np.where(max_qb < 1, 1, max_qb))


def parent_form(f16, qb, rows_min_qb):
    """launch_scan with form = -1: if (!f16 && qb >= 4 && qb >= rows_min_qb) the rows kernel, else by f16 the T16 or the one-row kernel"""
    return np.where(~f16 & (qb >= 4) & (qb >= rows_min_qb), ROWS, np.where(f16, T16, ONE))


def parent_launch(form, n, qb, dim, cus):
    """launch_scan's two grid rules and launch_scan_mq's: -> grid, threads, dynamic LDS bytes"""
    want = cdiv(np.where(form == T16, cdiv(n, 16), n), 4)           # want = cdiv64(f16 ? cdiv64(n, 16) : n, SCAN_WAVES)
    grid = np.maximum(np.where(want < cus * 8, want, cus * 8), 1)
    want_g = cdiv(cdiv(n, 4), 4)                                    # want_g = cdiv64(cdiv64(n, R), SCAN_WAVES)
    grid_g = np.maximum(np.where(want_g < cus * 8, want_g, cus * 8), 1)
    blocks = cdiv(cdiv(n, 16), 8 * 4)                               # blocks = cdiv64(tiles, MQ_WAVES * MQ_RT); grid = blocks < cus ? blocks : cus
    grid_mq = np.where(blocks < cus, blocks, cus)
    return (np.where(form == MQ, grid_mq, np.where(form == ROWS, grid_g, grid)), np.where(form == MQ, 512, 256),
            np.where(form == MQ, 2 * (2 * 64 * 256 * 2), qb * dim * 4))


def parent_passes(nq, width, mq, f16, rows_min_qb):
    """the scan loops of search_dev: for (q0 = 0; q0 < nq; q0 += width) { qb = nq - q0 < width ? nq - q0 : width; ... } -> [(q0, qb, form)]"""
    out, q0 = [], 0
    while q0 < nq:
        qb = nq - q0 if nq - q0 < width else width
        out.append((q0, qb, MQ if mq else int(parent_form(np.bool_(f16), qb, rows_min_qb))))
        q0 += width
    return out


def _expected(r):
    """the parent's search_dev, variable by variable"""
    n, nq, k, dim = r["n"], r["nq"], r["k"], r["dim"]
    f16 = r["storage"] == F16
    mq_min_queries = np.where(r["mq_min"] <= 0, 1 << 30, r["mq_min"])
    chunks = cdiv(np.where(n > 0, n, 1), 2048)
    per_q = np.where(n > chunks * k, n, chunks * k)
    kp = np.where(k + 24 > 2 * k, k + 24, 2 * k)
    mirror_path = (n >= r["mirror_min"]) & (n > 0) & (r["storage"] == F32) & (r["mirror"] != 0) & (nq >= mq_min_queries) & (nq <= 64) & (kp <= 64)
    mq = f16 & (nq >= mq_min_queries)
    max_qb = parent_query_block(dim)
    e = {"kp": kp, "per_q": per_q, "keys_bytes": nq * per_q * 8}
    e["path"] = np.where(mirror_path, MIRROR_CERT, np.where((n > 0) & mq, MQ_F16, EXACT_SCAN))
    e["cert_keys_bytes"] = np.where(mirror_path, nq * kp * 8, 0)
    e["cert_flags_bytes"] = e["hflags_bytes"] = np.where(mirror_path, 64 * 4, 0)
    on_mq = mirror_path | (mq & (n > 0))                            # the mirror pass is ONE launch_scan_mq of all nq <= 64 queries; `mq` lives inside if (n > 0)
    e["mq"] = on_mq
    e["width"] = np.where(on_mq, 64, max_qb)
    scanned = np.where(n > 0, nq, 0)                                # if (n > 0) { ... }: nothing is scanned over an empty index
    # the pass lists by the parent's literal loops, once per distinct (queries, width, matrix cores, storage, rows threshold)
    key = np.stack([scanned, e["width"], on_mq, f16, r["rows_min"]], 1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    summ = np.zeros((len(uniq), 10), np.int64)
    for i, (q, w, m, h, rm) in enumerate(uniq):
        p = parent_passes(int(q), int(w), bool(m), bool(h), int(rm))
        forms = [f for _, _, f in p]
        first, last = (p[0], p[-1]) if p else ((0, 0, 0), (0, 0, 0))
        summ[i] = [len(p), sum(a for a, _, _ in p), sum(b for _, b, _ in p), forms.count(ONE), forms.count(ROWS), forms.count(T16), forms.count(MQ), first[2], last[0],
                   last[1]]
    s = summ[inv.ravel()]
    for j, name in enumerate(["count", "sum_q0", "sum_qb", "n_one", "n_rows", "n_t16", "n_mq", "first_form", "last_q0", "last_qb"]):
        e[name] = s[:, j]
    some = e["count"] > 0
    first_qb = np.minimum(scanned, e["width"])
    e["last_form"] = np.where(some, np.where(on_mq, MQ, parent_form(f16, e["last_qb"], r["rows_min"])), 0)
    e["first_grid"] = np.where(some, parent_launch(e["first_form"], n, first_qb, dim, r["n_cu"])[0], 0)
    g, t, sm = parent_launch(e["last_form"], n, e["last_qb"], dim, r["n_cu"])
    e["last_grid"], e["last_threads"], e["last_smem"] = np.where(some, g, 0), np.where(some, t, 0), np.where(some, sm, 0)
    return e


def test_every_combination_matches_the_rules_restated(rows):
    exp = _expected(rows)
    assert sorted(exp) == sorted(set(ROW.names) - set(INPUTS))
    for name, want in exp.items():
        bad = np.flatnonzero(rows[name] != want.astype(np.int64))
        assert len(bad) == 0, (name, len(bad), {k: int(rows[k][bad[0]]) for k in INPUTS}, int(rows[name][bad[0]]), int(want[bad[0]]))
    # every path and every kernel occurs, and every query is scanned exactly once
    assert set(np.unique(rows["path"])) == {MIRROR_CERT, MQ_F16, EXACT_SCAN}
    assert all(rows[c].max() > 0 for c in ("n_one", "n_rows", "n_t16", "n_mq"))
    assert np.array_equal(rows["sum_qb"], np.where(rows["n"] > 0, rows["nq"], 0))
    # what a fact must not influence: the compute units choose no path and no pass, the mirror nothing on an fp16 shard
    shape = [2, 2, len(DIMS), len(NQS), len(KS), len(NS), len(MQ_MINS), len(ROWS_MINS), len(MIRROR_MINS), len(CUS)]
    for name in ("path", "kp", "per_q", "count", "width", "last_qb", "last_form", "last_smem"):
        a = rows[name].reshape(shape)
        assert (a == a[..., :1]).all(), name
        assert (a[F16, 0] == a[F16, 1]).all(), name


def _row(rows, **kw):
    d = dict(dim=4096, k=5, mq_min=4, rows_min=4, mirror_min=32768, n_cu=256)          # the production defaults (test_the_defaults_are_the_tables) on an MI355X
    d.update(kw)
    sel = np.ones(len(rows["path"]), bool)
    for k, v in d.items():
        sel &= rows[k] == v
    i, = np.flatnonzero(sel)
    return {n: int(rows[n][i]) for n in ROW.names}


def test_pinned_rows_of_the_benchmark_shapes(rows):
    for n in (100000, 125000, 400000):
        p = _row(rows, storage=F32, mirror=1, nq=1, n=n)                  # loop_match / roofline_knn: one query, fp32 rows
        assert (p["path"], p["count"], p["last_form"], p["last_grid"], p["last_threads"], p["last_smem"]) == (EXACT_SCAN, 1, ONE, 2048, 256, 16384)
        assert (p["per_q"], p["keys_bytes"], p["cert_keys_bytes"]) == (n, n * 8, 0)
        p = _row(rows, storage=F32, mirror=1, nq=64, n=n)                 # roofline_knn_batched on fp32 rows: the mirror, k + 24 candidates
        assert (p["path"], p["kp"], p["count"], p["last_form"], p["last_qb"], p["last_threads"], p["last_smem"]) == (MIRROR_CERT, 29, 1, MQ, 64, 512, 131072)
        assert p["last_grid"] == min(-(-n // 512), 256) and (p["cert_keys_bytes"], p["cert_flags_bytes"], p["hflags_bytes"]) == (64 * 29 * 8, 256, 256)
        p = _row(rows, storage=F32, mirror=0, nq=64, n=n)                 # a sharded fp32 index (no mirror): 8 passes of the rows kernel
        assert (p["path"], p["count"], p["width"], p["n_rows"], p["last_smem"], p["last_grid"]) == (EXACT_SCAN, 8, 8, 8, 131072, 2048)
        p = _row(rows, storage=F16, mirror=0, nq=1, n=n)                  # fp16 shard, one query: the VALU kernel over 16-row blocks
        assert (p["path"], p["count"], p["last_form"], p["last_grid"]) == (EXACT_SCAN, 1, T16, min(-(-(-(-n // 16)) // 4), 2048))
        p = _row(rows, storage=F16, mirror=0, nq=64, n=n)                 # fp16 shard, 64 key frames: one pass on the matrix cores
        assert (p["path"], p["count"], p["last_form"], p["last_qb"], p["last_grid"]) == (MQ_F16, 1, MQ, 64, min(-(-n // 512), 256))
    p = _row(rows, storage=F32, mirror=1, nq=64, n=100000, k=33)          # 2k = 66 candidates do not fit the select kernel: the exact passes
    assert (p["path"], p["kp"], p["n_rows"]) == (EXACT_SCAN, 66, 8)
    p = _row(rows, storage=F32, mirror=1, nq=64, n=32767)                 # below the production threshold
    assert p["path"] == EXACT_SCAN and _row(rows, storage=F32, mirror=1, nq=64, n=32767, mirror_min=0)["path"] == MIRROR_CERT
    p = _row(rows, storage=F32, mirror=1, nq=3, n=100000)                 # below OMNI_MQ_MIN: one pass of the one-row kernel
    assert (p["path"], p["count"], p["last_form"], p["last_qb"]) == (EXACT_SCAN, 1, ONE, 3)
    p = _row(rows, storage=F32, mirror=1, nq=9, n=400000, dim=8192)       # query block 4: 4 + 4 on the rows kernel, 1 on the one-row kernel
    assert (p["path"], p["kp"]) == (MIRROR_CERT, 29)
    p = _row(rows, storage=F32, mirror=0, nq=9, n=400000, dim=8192)
    assert (p["width"], p["count"], p["n_rows"], p["n_one"], p["last_q0"], p["last_qb"]) == (4, 3, 2, 1, 8, 1)
    p = _row(rows, storage=F16, mirror=0, nq=130, n=400000)               # 64 + 64 + 2 on the matrix cores
    assert (p["path"], p["count"], p["n_mq"], p["last_q0"], p["last_qb"]) == (MQ_F16, 3, 3, 128, 2)
    p = _row(rows, storage=F16, mirror=0, nq=64, n=0)                     # an empty index: no pass, the top-k still sized
    assert (p["path"], p["count"], p["per_q"]) == (EXACT_SCAN, 0, 5)


def test_every_pass_and_the_fallback_passes(pin):
    seen = 0
    for line in text(pin, "passes"):
        dim, mq, rows_min, nq, count = (int(v) for v in line[:5])
        got = [tuple(int(v) for v in line[5 + 3 * i:8 + 3 * i]) for i in range(count)]
        assert len(line) == 5 + 3 * count
        # mq 2: fallback_passes(nfl) of a mirror search -- the exact loop over the staged queries of an fp32 shard
        want = parent_passes(nq, 64 if mq == 1 else int(parent_query_block(dim)), mq == 1, mq == 1, rows_min)
        assert got == want, (dim, mq, rows_min, nq)
        seen += mq == 2
    assert seen == 4 * 64


def test_every_launch_and_form(pin):
    t = np.array([[int(v) for v in line] for line in text(pin, "launch") if line[0] != "mqbytes"], np.int64)
    form, dim, cus, n, qb = t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4]
    assert len(t) == 4 * len(DIMS) * len(CUS) * (len(NS) - 1) * 8 and n.min() == 1
    for got, want in zip((t[:, 5], t[:, 6], t[:, 7]), parent_launch(form, n, qb, dim, cus)):
        assert np.array_equal(got, want)
    assert (t[:, 5] >= 1).all()                                       # no empty grid
    assert [line[1:] for line in text(pin, "launch") if line[0] == "mqbytes"] == [[str(d), str(d // 256 * 65536)] for d in DIMS]       # slices * MQ_SLICE_BYTES
    f = np.array(text(pin, "forms"), np.int64)
    assert len(f) == 2 * 4 * 8 and np.array_equal(f[:, 3], parent_form(f[:, 0] == F16, f[:, 2], f[:, 1]))
    qblock = {int(a): int(b) for a, b in text(pin, "qblock")}
    assert all(v == int(parent_query_block(d)) for d, v in qblock.items())
    assert (qblock[512], qblock[4096], qblock[8192], qblock[32768], qblock[65536]) == (8, 8, 4, 1, 1)       # 8192: the smallest block of the rows kernel; the lower clamp


def test_capacity_rule(pin):
    lines = text(pin, "capacity")
    grown = [[int(v) for v in line] for line in lines if line[0] != "loaded"]
    assert len(grown) == 8 * 16
    for capacity, need, got in grown:
        if need <= capacity:                                            # ensure_capacity: if (rows <= ix->capacity) return OMNI_OK
            assert got == capacity
            continue
        cap = capacity if capacity > 0 else 1024
        while cap < need:
            cap *= 2
        assert got == (cap + 15) & ~15, (capacity, need)
    at = {(c, r): g for c, r, g in grown}
    assert at[(0, 1)] == 1024 and at[(0, 1025)] == 2048 and at[(1024, 1030)] == 2048 and at[(1000, 1030)] == 2000 and at[(1000, 3000001)] == 4096000
    for _, ntotal, got in (line for line in lines if line[0] == "loaded"):
        assert int(got) == ((max(int(ntotal), 1) + 15) & ~15)           # omni_index_load: cap = ((h.ntotal > 0 ? h.ntotal : 1) + 15) & ~15


def test_the_defaults_are_the_tables(pin):
    cfg = open(os.path.join(CSRC, "config.hip")).read()
    for env, default in (("OMNI_SCAN_ROWS_MIN", ROWS_MINS[0]), ("OMNI_MQ_MIN", MQ_MINS[-1]), ("OMNI_INDEX_MIRROR_MIN_ROWS", MIRROR_MINS[-1])):
        assert re.search(r'\{"%s", (\d+),' % env, cfg).group(1) == str(default), env
    sizes = {k: int(v) for k, v in text(pin, "sizes")}
    assert sizes == dict(SCAN_THREADS=256, SCAN_WAVES=4, SCAN_MAX_QB=8, SCAN_ROWS_R=4, MQ_THREADS=512, MQ_WAVES=8, MQ_RT=4, MQ_NQ=64, MQ_KS=256, MQ_SLICE_BYTES=65536,
                         MQ_SMEM=131072, INDEX_QUERY_LDS_BYTES=131072, TOPK_CHUNK=2048, TOPK_MAX_K=1024, TOPK_SEL_MAX_K=64)


def _body(src, name):
    """the definition of the function `name` (a line in column 0 that holds its signature and opens a brace) up to the closing brace in column 0"""
    m = re.search(r"^[^\s/][^\n;]*\b%s\([^;{]*\{\n.*?^\}\n" % name, src, re.S | re.M)
    assert m, name
    return m.group(0)


def test_the_host_code_decides_nothing_next_to_the_plan():
    src = open(os.path.join(CSRC, "index.hip")).read()
    owner = re.search(r"^struct IndexRows \{\n.*?^\};\n", src, re.S | re.M).group(0)
    rest = src.replace(owner, "")
    # one owner of the rows: nothing else allocates or frees device memory by hand, and nothing else assigns the three pointers
    assert owner.count("hipMalloc(") == 5 and not re.search(r"hipMalloc\(\s*[&(]", rest) and "hipFree(" not in rest      # (load's message says "hipMalloc(%zu)")
    assert not re.search(r"(->|\.)(db|db16|norm_max|capacity)\s*=[^=]", rest)
    for fn in ("ensure_capacity", "omni_index_load", "omni_index_set_shard", "omni_index_create", "omni_index_destroy"):
        assert "ix->rows." in _body(src, fn), fn
    # no literal copy of a size
    assert "131072" not in src
    sizes = "SCAN_THREADS|SCAN_WAVES|SCAN_MAX_QB|MQ_THREADS|MQ_WAVES|MQ_RT|MQ_NQ|MQ_KS|MQ_SLICE_BYTES|MQ_SMEM|TOPK_CHUNK|TOPK_MAX_K|TOPK_SEL_MAX_K"
    for name in ("index.hip", "topk.h"):
        assert not re.search(r"#define\s+(%s)\b" % sizes, open(os.path.join(CSRC, name)).read()), name
    # search_dev switches over the plan and decides nothing itself; the launchers take the plan's launch
    body = _body(src, "search_dev")
    for word in ("storage ==", "OMNI_STORE_", "mq_min", "TOPK_", "MQ_NQ", "SCAN_MAX_QB", "db16 &&"):
        assert word not in body, word
    assert "index_search_plan(index_facts(ix), nq, k, n)" in body and "switch (plan.path)" in body
    for fn in ("launch_scan", "launch_scan_mq"):
        body = _body(src, fn)
        assert "index_scan_launch(" in body and "multiProcessorCount" not in body and "cdiv" not in body and "= -1" not in body, fn
    assert src.count("multiProcessorCount") == 1 and src.count("run_scan_passes(") == 3          # its definition, the search, the certificate's fallback
    # plain host C++: nothing of HIP in the plan's headers
    for name in ("index_plan.h", "topk_sizes.h"):
        plan = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in plan and "__device__" not in plan and "common.h" not in plan, name
