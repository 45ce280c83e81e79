"""
The radix-sort edge cases of tests/radix_cases.py, without a GPU: every case satisfies the preconditions that put it on its
edge, and the plain NumPy reference (ref_sort: a stable argsort and a bincount running sum) returns exactly what the oracle
does -- row pointers with their dtype, indices, the values' bits -- so the two references agree before the library is asked.
Case F (3.4e7 records) is the one exception: a NumPy stable argsort of it takes several seconds, so the oracle's output is
checked there by the two properties that determine it, both O(n).
"""
import numpy as np
import pytest

import radix_cases as R


def _bits(v):
    return v.view(np.int64 if v.dtype == np.float64 else np.int32)


def _same(got, want, what):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert np.array_equal(got, want), what


def _same_values(got, want, what):
    if want is None:
        assert got is None, what
    else:
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), what


def test_registry_holds_every_family():
    count = {f: len(R.names(f + '-')) for f in 'ABCDEFG'}
    assert count == {'A': 20, 'B': 6, 'C': 51, 'D': 13, 'E': 18, 'F': 1, 'G': 12}
    assert len(R.CASES) == sum(count.values())


def test_route_rule():
    "the restated rule at its own edges (sort_records: bits = ceil(log2(key range)), packed iff two passes and payloads <= 2^24)"
    got = [R.route(k, 1000) for k, _ in R.LADDER]
    assert got == [e for _, e in R.LADDER] == ['1', '1', '1', '1', 'packed', 'packed', 'packed', '3', '3', '4']
    assert R.route(65536, R.P24) == 'packed' and R.route(65536, R.P24 + 1) == 'plain2'
    assert R.route(257, R.P24 + 1) == 'plain2' and R.route(256, R.P24 + 1) == '1' and R.route(65537, R.P24 + 1) == '3'


def test_reference_on_hand_written_records():
    ptr, pay, vs = R.ref_sort(np.array([2, 0, 2, 1, 0]), np.array([10, 11, 12, 13, 14]), np.array([1, 2, 3, 4, 5], np.float32), 4)
    assert ptr.tolist() == [0, 2, 3, 5, 5] and pay.tolist() == [11, 14, 13, 10, 12]
    assert vs.dtype == np.float64 and vs.tolist() == [2, 5, 4, 1, 3]
    rp, ci, v = R.ref_transpose(2, 3, np.array([0, 2, 3], np.int64), np.array([2, 0, 2], np.int32), None)
    assert rp.dtype == np.int64 and rp.tolist() == [0, 1, 1, 3] and ci.tolist() == [0, 0, 1] and v is None
    rp, ci, v = R.ref_from_coo(3, np.array([2, 0, 2]), np.array([5, 6, 4]), np.array([1, 2, 3], np.float32))
    assert rp.dtype == np.int32 and rp.tolist() == [0, 1, 1, 3] and ci.tolist() == [6, 5, 4]
    assert v.dtype == np.float32 and v.tolist() == [2, 1, 3]
    ci, v = R.ref_order_columns(2, np.array([0, 3, 4]), np.array([5, 1, 5, 0], np.int32), np.array([1., 2., 3., 4.]))
    assert ci.tolist() == [1, 5, 5, 0] and v.tolist() == [2, 1, 3, 4]
    assert R.aligned_chunks(np.array([7] * 4097 + [263] + [8])) == 3


@pytest.mark.parametrize('name', [n for n in R.CASES if n != 'F-many-chunks'])
def test_case_holds_its_edge_and_references_agree(name):
    from oracle import oracle as O
    c = R.build(name)
    assert not R.failed_preconditions(c), (name, R.failed_preconditions(c))
    if c.op == 'transpose':
        rp, ci, vs = c.ref()
        nr, nc, orp, oci, ovs = O.transpose(c.nrows, c.ncols, c.rowptrs, c.colinds, c.values)
        assert (nr, nc) == (c.ncols, c.nrows) and rp.dtype == c.rowptrs.dtype
    elif c.op == 'from_coo':
        rp, ci, vs = c.ref()
        orp, oci, ovs = O.from_coo(c.nrows, c.rows, c.cols, c.values)
        assert rp.dtype == np.int32
    else:
        ci, vs = c.ref()
        oci, ovs = O.sort_rows(c.nrows, c.rowptrs, c.colinds, c.values)
        if ovs is not None:
            assert np.array_equal(ovs, vs.astype(np.float64))        # (the oracle's sort works on float64 copies: exact)
            ovs = vs
        # the same through two transposes, the way the library does it
        t = R.ref_transpose(c.nrows, c.ncols, c.rowptrs, c.colinds, c.values)
        rp, ci2, vs2 = R.ref_transpose(c.ncols, c.nrows, *t)
        orp = c.rowptrs
        assert np.array_equal(ci2, ci) and (vs is None or np.array_equal(_bits(vs2), _bits(vs.astype(np.float64))))
    _same(rp, orp, name)
    _same(ci, oci, name)
    _same_values(vs, ovs, name)
    if c.pre.get('the payload is the source index'):
        # stability, read directly off the output: source positions ascend inside every output row
        inner = np.ones(c.n, dtype=bool)
        inner[rp[1:-1][rp[1:-1] < c.n]] = False
        assert np.all((np.diff(ci) > 0) | ~inner[1:])


def test_many_chunks_case_by_properties():
    "F: the oracle's output is the counting sort's -- pointers = running sum of the row counts, source positions ascending inside rows"
    from oracle import oracle as O
    c = R.build('F-many-chunks')
    assert not R.failed_preconditions(c), R.failed_preconditions(c)
    assert c.values is None and np.array_equal(c.cols, np.arange(c.n, dtype=np.int32))
    rp, ci, vs = O.from_coo(c.nrows, c.rows, c.cols, None)
    assert vs is None and rp.dtype == np.int32 and ci.dtype == np.int32
    want = np.zeros(c.nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(c.rows, minlength=c.nrows), out=want[1:])
    assert np.array_equal(rp, want) and np.all(np.diff(want) > 0)
    # every output row holds entries of that row only, in ascending source position: there is one such arrangement
    assert np.array_equal(c.rows[ci], np.repeat(np.arange(c.nrows, dtype=np.int32), np.diff(want)))
    inner = np.ones(c.n, dtype=bool)
    inner[want[1:-1]] = False
    assert np.all((np.diff(ci) > 0) | ~inner[1:])
