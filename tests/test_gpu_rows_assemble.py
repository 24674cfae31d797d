"""rows_assemble_kernel (csrc/rows_assemble.hip) against omni_rows_assemble_host -- csrc/rows_plan.h under g++, itself pinned to numpy indexing by
tests/test_rows_plan_cpu.py -- bitwise as uint32, on that test's shapes: dim 4096 and 8 take the 16-byte path, 6 and 1 the dword path, 67 rows are 67 workgroups,
dim 4096 is four steps of a workgroup's 256 lanes and dim 6 / 1 leave most of them idle.  The tables mix the three sources and repeat source rows; NaN payloads,
-0.0 and a denormal are planted.  One more case takes the dword path by ALIGNMENT: dim 8 with the unit block one float off the 16-byte grid.  The output buffer is
pre-filled, so a row the kernel did not write shows."""
import numpy as np
import pytest

from tests.test_rows_plan_cpu import DIMS, ROWS, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_kernel_equals_the_host_assembly_bit_for_bit(omni, ctx, n_rows, dim):
    c = omni.capi
    table, unit, staged = case(c, n_rows, dim, 100 * dim + n_rows)
    want = c.rows_assemble_host(table, unit, staged, dim)
    got = c.rows_assemble(ctx, table, unit, staged, dim)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_dword_path_by_alignment(omni, ctx):
    c = omni.capi
    table, unit, staged = case(c, 67, 8, 5)
    want = c.rows_assemble_host(table, unit, staged, 8)
    got = c.rows_assemble(ctx, table, unit, staged, 8, unit_offset_floats=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_blocks_without_rows_and_an_entry_out_of_range(omni, ctx):
    """a batch of remote frames alone has no unit block; the kernel serves an entry its maker should have refused with zeros, and reads nothing for it"""
    c = omni.capi
    staged = np.arange(3 * 8, dtype=np.float32).reshape(3, 8) + 1
    table = np.array([[c.ROW_STAGED, 2], [c.ROW_ZERO, 0], [c.ROW_STAGED, 0], [c.ROW_UNIT, 0], [c.ROW_STAGED, 3], [7, 0]], np.int32)
    got = c.rows_assemble(ctx, table, np.zeros((0, 8), np.float32), staged, 8)
    zero = np.zeros(8, np.float32)
    assert np.array_equal(got, np.stack([staged[2], zero, staged[0], zero, zero, zero]))
