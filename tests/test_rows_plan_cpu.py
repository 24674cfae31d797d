"""CPU gate of the rows of a mixed detector batch (csrc/rows_plan.h, what csrc/rows_assemble.hip runs one workgroup per row): omni_rows_assemble_host -- the same
header inside libomni_hip.so, no GPU and no context -- against numpy indexing, bitwise as uint32 (NaN payloads, -0.0 and denormals are planted), for dim in
{4096, 8, 6, 1} and n_rows in {1, 5, 67}, tables that mix all three sources with repeated source rows; and every refusal, a code and a message before anything
is read."""
import numpy as np
import pytest

DIMS, ROWS = (4096, 8, 6, 1), (1, 5, 67)


def case(c, n_rows, dim, seed, n_unit=7, n_staged=5):
    """(table, unit rows, staged rows) with every source present (n_rows permitting), repeated source rows, and payload bits a float copy could lose"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, size=(n_unit + n_staged, dim), dtype=np.uint64).astype(np.uint32)
    bits[0, 0], bits[-1, -1] = 0x7FC01234, 0xFFA00001              # a quiet and a signalling NaN with payloads
    bits[1 % (n_unit + n_staged), 0] = 0x80000000                  # -0.0
    bits[2 % (n_unit + n_staged), -1] = 0x00000001                 # the smallest denormal
    unit, staged = bits[:n_unit].view(np.float32), bits[n_unit:].view(np.float32)
    source = rng.integers(0, 3, size=n_rows)
    source[:3] = [c.ROW_UNIT, c.ROW_STAGED, c.ROW_ZERO][:n_rows]
    index = np.where(source == c.ROW_UNIT, rng.integers(0, n_unit, size=n_rows), rng.integers(0, n_staged, size=n_rows))
    if n_rows >= 5:
        source[3], index[3], source[4], index[4] = source[0], index[0], source[1], index[1]      # the same source rows again
    return np.stack([source, index], 1).astype(np.int32), unit, staged


def expected_bits(c, table, unit, staged, dim):
    out = np.zeros((len(table), dim), np.uint32)
    for r, (s, i) in enumerate(table):
        if s == c.ROW_UNIT:
            out[r] = unit[i].view(np.uint32)
        elif s == c.ROW_STAGED:
            out[r] = staged[i].view(np.uint32)
    return out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_host_assembly_is_numpy_indexing_bit_for_bit(omni, n_rows, dim):
    c = omni.capi
    table, unit, staged = case(c, n_rows, dim, 100 * dim + n_rows)
    got = c.rows_assemble_host(table, unit, staged, dim)
    assert got.shape == (n_rows, dim) and np.array_equal(got.view(np.uint32), expected_bits(c, table, unit, staged, dim))
    if n_rows >= 5:
        assert {c.ROW_UNIT, c.ROW_STAGED, c.ROW_ZERO} <= set(table[:, 0].tolist())


def test_a_block_without_rows_may_be_absent(omni):
    c = omni.capi
    table = np.array([[c.ROW_ZERO, 0], [c.ROW_STAGED, 0], [c.ROW_ZERO, 123]], np.int32)      # (a ZERO entry's index is not read)
    staged = np.arange(8, dtype=np.float32)[None]
    got = c.rows_assemble_host(table, np.zeros((0, 8), np.float32), staged, 8)
    assert np.array_equal(got, np.stack([np.zeros(8, np.float32), staged[0], np.zeros(8, np.float32)]))


def test_every_refusal(omni):
    c = omni.capi
    L = c.lib()
    table, unit, staged = case(c, 5, 8, 1)
    out = np.full((5, 8), 3.0, np.float32)

    def call(tb=table, n_rows=5, dim=8, n_unit=len(unit), n_staged=len(staged), u=unit, s=staged, o=out):
        tb = None if tb is None else np.ascontiguousarray(tb, np.int32)
        rc = L.omni_rows_assemble_host(n_rows, dim, None if tb is None else tb.ctypes.data, None if u is None else u.ctypes.data, n_unit,
                                       None if s is None else s.ctypes.data, n_staged, None if o is None else o.ctypes.data)
        return rc, L.omni_last_error().decode()

    def with_entry(r, source, index):
        t = table.copy()
        t[r] = (source, index)
        return t

    assert call()[0] == c.OK
    for kw, word in (({"tb": None}, "null"), ({"o": None}, "null"), ({"n_rows": 0}, "n_rows"), ({"n_rows": -3}, "n_rows"), ({"dim": 0}, "dim"), ({"dim": -1}, "dim"),
                     ({"n_unit": -1}, "negative"), ({"n_staged": -1}, "negative"),
                     ({"tb": with_entry(2, c.ROW_UNIT, len(unit))}, "out of range"), ({"tb": with_entry(4, c.ROW_UNIT, -1)}, "out of range"),
                     ({"tb": with_entry(0, c.ROW_STAGED, len(staged))}, "out of range"), ({"tb": with_entry(1, c.ROW_STAGED, -2)}, "out of range"),
                     ({"tb": with_entry(3, 3, 0)}, "unknown row source"), ({"tb": with_entry(3, -1, 0)}, "unknown row source"),
                     ({"tb": with_entry(0, c.ROW_UNIT, 0), "n_unit": 0}, "out of range"),
                     ({"u": None}, "no address"), ({"s": None}, "no address")):
        out[:] = 3.0
        rc, msg = call(**kw)
        assert rc == c.ERR_INVALID and word in msg, (kw, rc, msg)
        assert np.all(out == 3.0)                                  # refused before anything was written
    # the device entry refuses what it can see without reading the table, before it touches the context
    fake = np.zeros(64, np.int64)
    for args, word in (((None, 5, 8, 1, 1, 7, 1, 5, 1), "null"), ((fake.ctypes.data, 5, 8, None, 1, 7, 1, 5, 1), "null"), ((fake.ctypes.data, 5, 8, 16, 16, 7, 16, 5, None), "null"),
                       ((fake.ctypes.data, 0, 8, 16, 16, 7, 16, 5, 16), "n_rows"), ((fake.ctypes.data, 5, 0, 16, 16, 7, 16, 5, 16), "dim"),
                       ((fake.ctypes.data, 5, 8, 16, None, 7, 16, 5, 16), "no address"), ((fake.ctypes.data, 5, 8, 16, 16, 7, None, 5, 16), "no address"),
                       ((fake.ctypes.data, 5, 8, 16, 18, 7, 16, 5, 16), "aligned")):
        assert L.omni_rows_assemble_enqueue_dev(*args) == c.ERR_INVALID and word in L.omni_last_error().decode(), args
    assert L.omni_memcpy_h2d_async(None, 16, 16, 4) == c.ERR_INVALID
