"""
The stable radix sort behind transpose, from_coo and order_columns (csrc/transpose.hip, sort_records) at every route, chunk
and run boundary, through the public entries K.transpose / K.from_coo / K.order_columns.  The cases and their preconditions
come from tests/radix_cases.py (tests/test_radix_cases_host.py checks them, and the NumPy reference against the oracle,
without a GPU); the preconditions are asserted again here before the library is asked.

All of it is index work and copied bits: every comparison -- row pointers with their dtype, column indices, the raw bits of the
values -- is exact.  The route sort_records takes is a function of the shape: bits = ceil(log2(key range)); one pass up to
8 bits, otherwise ceil(bits / 8); two passes with a payload range of at most 2^24 are the packed route (12-byte records, second
pass on chunks aligned to the first pass's runs), two passes beyond that the plain two-pass route.  transpose: key = column,
payload = source row (recovered from the row pointers inside the first pass); from_coo: key = row, payload = column.
"""
import numpy as np
import pytest

import radix_cases as R

pytestmark = pytest.mark.gpu


def _bits(v):
    return v.view(np.int64 if v.dtype == np.float64 else np.int32)


def _eq(got, want, what):
    assert got.dtype == want.dtype, f'{what}: dtype {got.dtype}, expected {want.dtype}'
    assert got.shape == want.shape, f'{what}: shape {got.shape}, expected {want.shape}'
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f'{what}: {int(np.count_nonzero(got != want))} of {got.size} differ, first at {at}: '
                             f'{got[at]} instead of {want[at]}')


def _eq_values(got, want, what):
    if want is None:
        assert got is None, f'{what}: values where none are expected'
    else:
        assert got is not None, f'{what}: no values'
        assert got.dtype == want.dtype, f'{what}: dtype {got.dtype}, expected {want.dtype}'
        _eq(_bits(got), _bits(want), what)


def _export(K, h):
    try:
        return K.from_handle(h)
    finally:
        K.release_handle(h)


def _run(name, c=None, ref=None):
    "build the case, check that it is on its edge, run it through its public entry and compare with the reference, bit for bit"
    from csr_amd import CSR
    from csr_amd.kernels import hip as K
    c = c or R.build(name)
    assert not R.failed_preconditions(c), (name, R.failed_preconditions(c))
    if c.op == 'from_coo':
        rp, ci, vs = ref or c.ref()
        out = _export(K, K.from_coo(c.rows, c.cols, c.values, (c.nrows, c.ncols)))
        assert (out.nrows, out.ncols, out.nnz) == (c.nrows, c.ncols, c.n), name
    else:
        m = CSR(c.nrows, c.ncols, c.n, c.rowptrs, c.colinds, c.values, _cast=False)
        h = K.to_handle(m)
        try:
            if c.op == 'transpose':
                rp, ci, vs = c.ref()
                out = _export(K, K.transpose(h))
                assert (out.nrows, out.ncols, out.nnz) == (c.ncols, c.nrows, c.n), name
            else:
                ci, vs = c.ref()
                rp = c.rowptrs                               # the handle's row pointers are unchanged
                K.order_columns(h)
                out = K.from_handle(h)
                assert (out.nrows, out.ncols, out.nnz) == (c.nrows, c.ncols, c.n), name
        finally:
            K.release_handle(h)
    _eq(out.rowptrs, rp, f'{name} rowptrs')
    _eq(out.colinds, ci, f'{name} colinds')
    _eq_values(out.values, vs, f'{name} values')
    return c


# ---- A ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('key_range', [r for r, _ in R.LADDER])
def test_key_range_ladder(key_range):
    """
    About 20 000 records with a key range of 1, 2, 255, 256 (one pass), 257, 65535, 65536 (two passes: packed, the payload
    ranges are 700 and 5000), 65537, 2^24 (three passes) and 2^24 + 1 (four passes), as a transpose with that many columns
    (float64 values) and as a from_coo with that many rows (structure only / float32 in turn).  The keys hold 0, the largest
    key, and whichever of 255, 256, 65535, 65536, 2^24 - 1, 2^24 the range admits: the last key of one digit count and the
    first of the next.
    """
    expect = dict(R.LADDER)[key_range]
    for op in ('transpose', 'from_coo'):
        c = _run(f'A-{op}-{key_range}')
        assert c.expect == expect


# ---- B ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.names('B-'))
def test_payload_edges_of_the_two_pass_routes(name):
    """
    Key range 65536 (two passes) with the payload range on both sides of the packed route's gate.  Payload range 2^24: the
    packed route with every bit of its word {high digit of the key in bits 31..24, payload in bits 23..0} in use -- key
    65535 with payload 2^24 - 1 is the word 0xffffffff, keys from 32768 on set its sign bit, payloads from 2^23 on bit 23.
    Payload range 2^24 + 1: the plain two-pass route (sorted keys written, row pointers read off them), payload 2^24 included.
    As a transpose (the payload is the source row: 2^24 or 2^24 + 1 rows, all entries in rows 0, 2^23 - 1, 2^23, 2^24 - 2,
    2^24 - 1 and 2^24, with int32 and with int64 row pointers) and as a from_coo (the payload is the column; int32 row
    pointers, the only width that entry produces below 2^31 entries).
    """
    c = _run(name)
    assert c.expect == ('packed' if str(R.P24 + 1) not in name else 'plain2')


# ---- C ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ncols,expect', R.COUNT_ROUTES)
def test_record_count_ladder(ncols, expect):
    """
    Record counts at every edge of the chunking, on the one-pass (100 columns), packed (1000) and three-pass (70 000) routes:
    1, 2, a wavefront's 64 and a round's 512 with their neighbours, one 4096-record chunk less one / exactly / plus one, the
    histogram's group of four chunks less one record / exactly / plus one, the scatter grid's eight chunks exactly and plus
    one record (a ninth chunk: seven padding workgroups return early), and 9 * 4096 + 5.  Values float64 / float32 / absent
    in turn, rows of 0 .. 40 entries.
    """
    for n in R.COUNTS:
        c = _run(f'C-{ncols}-{n}')
        assert c.expect == expect and c.n == n, n


# ---- D ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.names('D-'))
def test_run_shapes_of_the_aligned_second_pass(name):
    """
    Packed route (from_coo, 65536 rows, the column is the entry's position in the input, so a stability fault shows as a
    descent inside a row).  The second pass cuts every run of equal low digits into chunks of its own (rx_align_kernel) and
    reads the row pointers off its digit table (rx_rowptr_from_table_kernel); its descriptor arrays hold ceil(n / 4096) + 256
    chunks.  Runs it has to cut: one key only (one run over four chunks; keys 0, 255, 256, 65535); 256 runs of one record
    (256 aligned chunks against one plain chunk); every run 1 or 4097 long (ceil(n / 4096) + 255 aligned chunks, the most
    the arrays can be asked for); runs of exactly 4096 and 8192 between empty digits; one populated low digit (0: 255 trailing
    empty runs, 255: 255 leading ones); keys that are multiples of 256, keys all below 256; ascending and descending input.
    """
    c = _run(name)
    assert c.expect == 'packed'


# ---- E ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.names('E-'))
def test_source_row_recovery(name):
    """
    Packed route, 1000 columns, int32 and int64 row pointers.  The first pass of a transpose recovers every entry's source row
    per 4096-entry chunk: the first and last row meeting the chunk (rx_rowbounds_kernel), each of those rows' first entries
    marked with the row's id in LDS (the largest id wins where empty rows share a position) and a running maximum.  One row
    over four chunks between 10 000 empty rows on either side; 8292 rows of one entry; rows starting on entries 4095, 4096,
    4097 and 8192; 5000 empty rows sharing a chunk's first entry (4096) or its last (4095) with the row that follows them; a
    single row; leading-only and trailing-only empty rows; 20 000 rows of which one in five holds one entry, all meeting
    one chunk.
    """
    c = _run(name)
    assert c.expect == 'packed'


# ---- F ---------------------------------------------------------------------------------------------------------------------

def test_more_than_8192_chunks():
    """
    One pass (200 rows), structure only, 8192 * 4096 + 4097 entries: 8194 chunks, so the scan of the (digit, chunk) table
    (rx_scan_kernel, 8192 chunks per trip) makes a second trip and carries its running sum over; the last chunk holds one
    record.  Rows are a multiplicative hash of the entry's position, the column is the position.  Against the oracle.
    """
    from oracle import oracle as O
    c = R.build('F-many-chunks')
    ref = O.from_coo(c.nrows, c.rows, c.cols, None)
    assert ref[0].dtype == np.int32 and ref[2] is None
    _run('F-many-chunks', c, ref)
    assert c.expect == '1'


# ---- G ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.names('G-'))
def test_order_columns_two_routes(name):
    """
    order_columns is two transposes, and their key ranges are the matrix's two dimensions: 300 x 70 000 (three passes, then
    packed), 70 000 x 200 (one pass, then three), 100 x 100 (one pass twice, rows holding columns twice), 65536 x 65536 (packed
    twice, entry (65535, 65535) present).  Float64, float32 (comes back float32 with the same bits) and absent values.  Expected:
    every row sorted by column, equal columns in their stored order; the row pointers as they were.
    """
    c = _run(name)
    assert c.expect == dict((f'{nr}x{nc}', e) for nr, nc, _, e in R.ORDER_SHAPES)[name.split('-')[1]]
