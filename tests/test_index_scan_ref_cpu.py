"""CPU: the references of tests/index_scan_ref.py judge themselves before they judge the GPU (no GPU, no library).

The float32 emulations of the scan kernels lie inside tier 1 at every shape family of tests/test_gpu_index_scores.py (reduced n); every defect restated in the
emulations fails tier 2 in its class; cert_eps covers the worst-case row's loss and is no more than twice it; the victim scene of the end-to-end certificate test
has the margins that test relies on.

Defect ratios (RMS(z_defect) / RMS(z_clean) in the defect's worst class; matrix cores: dim 4096, 64 queries, 17 blocks of 512 rows, rotation on, classes of
>= 1 000 scores; printed with -s).  Every one must be >= 5 x the largest gate of index_scan_ref.TIER2_C (5 x 8.57 = 42.9); no class or shape had to be narrowed:
  lo operand dropped for one k-step                                     68.4   (query slot 9)
  lo operand dropped for one k-step of the query fragment 16 .. 31      68.0   (query slot 18)      <- the smallest
  one k-step's query operands read from the previous slice's buffer     4.7e5  (query slot 23)
  one 16-row tile scored with the clamped last tile's rows              1.6e6  (tile place 5)
  the rotation ignored by one block's row pointers                      6.3e7  (tile place 24)
  inv applied twice for the slot next to the padding                    3.7e6  (query slot 63)
  a lane's last fmaf missing in the VALU chain                          1.0e6 at dim 512, 2.1e5 at dim 4096 (query slot)
SMALLEST_DEFECT_RATIO below is asserted against the run.
"""
import numpy as np
import pytest

from tests import index_scan_ref as R

MIN_DEFECT_RATIO = 5.0 * max(R.TIER2_C.values())
SMALLEST_DEFECT_RATIO = 67.9           # lo_fragment; the condition of the gates: SMALLEST_DEFECT_RATIO >= MIN_DEFECT_RATIO


def test_the_gates_leave_every_defect_five_times_outside():
    assert SMALLEST_DEFECT_RATIO >= MIN_DEFECT_RATIO


@pytest.mark.parametrize("dim,n", [(512, 1027), (4096, 1027), (512, 5)])
def test_fp32_emulation_inside_tier1(dim, n):
    rows = R.unit_rows(n, dim, seed=dim + n)
    q = R.queries(rows, 8, seed=1, special=False)
    ref, em = R.f32_ref(q, rows), R.valu_emul(q, rows)
    assert R.tier1(em, ref) <= 1.0
    assert np.abs(em - ref.y).max() > 0 or n < 16               # an emulation, not a copy of the ideal
    t2 = R.tier2(em, em, ref, R.valu_classes(8, n, 4))
    assert t2["ratio"] in (0.0, 1.0) and (t2["judged"] > 0) == (8 * n >= R.MIN_CLASS)


@pytest.mark.parametrize("dim,n", [(512, 1000), (4096, 1000), (512, 17)])
def test_fp16_valu_emulation_inside_tier1(dim, n):
    rows16 = R.h16(R.unit_rows(n, dim, seed=dim + n + 1))
    q = R.queries(rows16, 8, seed=2, special=False)
    assert R.tier1(R.t16_emul(q, rows16), R.t16_ref(q, rows16)) <= 1.0


@pytest.mark.parametrize("dim,n,nq,rotate", [(4096, 16 * 512 + 83, 64, True), (4096, 1029, 63, False), (512, 2 * 4 * 512 + 512 * 7 + 16 * 9 + 3, 64, True),
                                             (1024, 2 * 4 * 512 + 512 * 7 + 16 * 9 + 3, 4, True), (4096, 17, 1, True)])
def test_matrix_core_emulation_inside_tier1(dim, n, nq, rotate):
    rows16 = R.h16(R.unit_rows(n, dim, seed=dim + n + 2))
    q = R.queries(rows16, nq, seed=3, special=True)
    ref, em = R.mq_ref(q, rows16), R.mq_emul(q, rows16, rotate)
    assert R.tier1(em, ref) <= 1.0
    if nq >= 4:
        assert (em[3] == 0).all() and (ref.E[3] == 0).all()      # the zero query: exact zeros, allowance 0
    # the residue allowance is the smaller part: tier 1 is about the summation
    assert (ref.E <= 1.01 * R.gamma(2 * dim) * ref.T + 1e-300)[ref.T > 0].all() or nq >= 6      # (slot 4's subnormal lo halves make R the larger part there)


def test_prep_restates_the_split():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((6, 512)).astype(np.float32)
    q[1] *= np.float32(1e30)
    q[2] = 0
    q[3] *= np.float32(1e-32)
    hi, lo, v, inv = R.mq_prep(q)
    m = np.abs(v).max(axis=1)
    assert (m[[0, 1, 4, 5]] >= 2.0 ** 13).all() and (m[[0, 1, 4, 5]] < 2.0 ** 14).all()       # max |q| lands in [2^13, 2^14)
    assert inv[2] == 1 and (hi[2] == 0).all() and inv[3] == np.float32(2.0 ** -100)            # m == 0; the clamped shift
    assert (np.abs(v - hi - lo) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
    assert np.array_equal((v[0] * float(inv[0])).astype(np.float32), q[0])


def test_keys_restate_the_order():
    s = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    keys = R.make_keys(s, np.arange(8))
    assert (np.diff(keys.astype(object)) > 0).all()                                           # ascending scores, -0 below +0: ascending keys
    sc, rows, empty = R.decode_keys(keys)
    assert np.array_equal(sc.view(np.uint32), s.view(np.uint32)) and np.array_equal(rows, np.arange(8)) and not empty.any()
    assert R.make_keys(np.float32([1.0, 1.0]), [4, 5])[0] > R.make_keys(np.float32([1.0, 1.0]), [4, 5])[1]      # ties: the lower row first
    assert R.decode_keys(np.array([0], np.uint64))[2].all()


@pytest.fixture(scope="module")
def mq_scene():
    dim, n, nq = 4096, 16 * 512 + 83, 64
    rows16 = R.h16(R.unit_rows(n, dim, seed=11))
    q = R.queries(rows16, nq, seed=12, special=True)
    ref = R.mq_ref(q, rows16)
    return q, rows16, ref, R.mq_emul(q, rows16, True), R.mq_classes(nq, n, grid=8)


@pytest.mark.parametrize("defect", R.MQ_DEFECTS)
def test_every_matrix_core_defect_fails_tier2(mq_scene, defect):
    q, rows16, ref, clean, classes = mq_scene
    t2 = R.tier2(R.mq_emul(q, rows16, True, defect), clean, ref, classes)
    print(f"defect {defect}: ratio {t2['ratio']:.4g} in {t2['where']}")
    assert t2["ratio"] >= MIN_DEFECT_RATIO and t2["ratio"] >= SMALLEST_DEFECT_RATIO, (defect, t2)
    assert R.tier2(clean, clean, ref, classes)["ratio"] == 1.0


def test_the_valu_defect_fails_tier2():
    for dim in (512, 4096):
        rows = R.unit_rows(1027, dim, seed=21)
        q = R.queries(rows, 8, seed=22, special=False)
        ref, clean = R.f32_ref(q, rows), R.valu_emul(q, rows)
        t2 = R.tier2(R.valu_emul(q, rows, "last_fmaf"), clean, ref, R.valu_classes(8, 1027, 4))
        print(f"defect last_fmaf, dim {dim}: ratio {t2['ratio']:.4g} in {t2['where']}")
        assert t2["ratio"] >= MIN_DEFECT_RATIO, t2


@pytest.mark.parametrize("dim", [512, 4096])
def test_cert_eps_covers_the_worst_case_row_and_no_more_than_twice(dim):
    v = R.worst_case_row(dim, seed=5)
    v64 = v.astype(np.float64)
    q = (v64 / np.linalg.norm(v64)).astype(np.float32)
    gap = abs(float(q.astype(np.float64) @ (v64 - R.h16(v).astype(np.float64))))
    qv = np.linalg.norm(q.astype(np.float64)) * np.linalg.norm(v64)
    eps = float(R.cert_eps(q[None], v[None])[0])
    print(f"dim {dim}: gap {gap / qv:.4e} |q||row|, eps {eps / qv:.4e} |q||row|")
    assert abs(gap / qv - 4.80e-4) < 0.01e-4
    assert gap <= eps < 2 * gap
    assert np.isinf(R.cert_eps(q[None] * np.float32(1e-20), v[None])).all() and np.isinf(R.cert_eps(q[None], v[None] * np.float32(1e6))).all()
    assert 0.5 * eps < gap                                       # the mutation the GPU victim test exists for: half the eps no longer covers the row


@pytest.mark.parametrize("k", [1, 10])
def test_victim_scene_has_its_margins(k):
    rows, q, victim, fillers = R.victim_scene(4096, k, seed=40 + k)
    kp = max(k + 24, 2 * k)
    assert len(fillers) == kp - k + 1 and len(set(fillers.tolist()) | {victim}) == len(fillers) + 1
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    exact, mirror = r64 @ q64, R.h16(rows).astype(np.float64) @ q64
    assert np.array_equal(R.h16(rows[fillers]), rows[fillers])                                 # exactly representable in fp16
    assert (np.linalg.norm(r64[fillers], axis=1) <= np.linalg.norm(r64[victim])).all()
    assert (mirror[fillers] - mirror[victim] >= 1e-5).all() and (exact[victim] - exact[fillers] >= 1e-5).all()
    lo, hi = mirror[victim], exact[victim]
    assert (exact[fillers] >= lo + 0.1 * (hi - lo) - 1e-6).all() and (exact[fillers] <= lo + 0.9 * (hi - lo) + 1e-6).all()
    ids, _ = R.oracle_topk(q[None], rows, k)
    assert ids[0, k - 1] == victim                                                             # the true k-th neighbour
    order = np.argsort(-mirror, kind="stable")
    assert victim not in order[:kp].tolist() and set(fillers.tolist()) <= set(order[:kp].tolist())      # the mirror's candidates: every filler, not the victim
    # what the certificate sees: kth = the best filler's exact score, m = the kp-th mirror score; sound eps refuses, half of it would certify
    kth, m, eps = exact[fillers].max(), mirror[order[kp - 1]], float(R.cert_eps(q[None], rows)[0])
    assert not kth > m + eps + 1e-5 and kth > m + 0.5 * eps + 1e-5
