"""
The refusals of the dense-panel operations, pinned word for word, without a GPU.

C side (tests/panel_refusal_cases.py has the tables): what needs no handle -- csrk_solve_blocks, csrk_topk_scores with
seen = 0, the scalars csrk_rank_entries looks at before its handles, and every entry's answer to an invalid handle -- each
through the host and the _device entry: the return code, the exact csrk_last_error() text, nothing written.

Python side (csr_amd/kernels/hip.py): every case of the _bad() tables of the sddmm, gram, als, topk_scores and rank_entries
host tests with its exact ValueError text, and requests that are wrong in two ways, which pin the order of the checks.
The texts are literals; none is produced by the code under test.
"""
import numpy as np
import pytest

import panel_refusal_cases as P
import test_als_host
import test_gram_host
import test_rank_entries_host
import test_sddmm_host
import test_topk_scores_host


# ---- C side --------------------------------------------------------------------------------------------------------------

def _buffers():
    "(host buffers, buffers for the _device entries): on the card where there is one, so that a lost refusal faults nothing"
    import torch
    return P.Buffers(False), P.Buffers(torch.cuda.is_available())


@pytest.mark.parametrize('table', P.NO_HANDLE)
def test_c_refusals_that_need_no_handle(table):
    from csr_amd._lib import lib
    host, dev = _buffers()
    P.run_table(lib, table, table, host, dev, {'mat': 0})


@pytest.mark.parametrize('entry', ['csrk_spmm_dense', 'csrk_sddmm', 'csrk_gram_rows', 'csrk_als_rows'])
def test_c_invalid_handles(entry):
    from csr_amd._lib import lib
    host, dev = _buffers()
    P.run_table(lib, entry, entry, host, dev, {}, only='invalid handle')


def test_c_invalid_seen_handle():
    from csr_amd._lib import lib
    host, dev = _buffers()
    P.run_table(lib, 'csrk_topk_scores with seen', 'csrk_topk_scores', host, dev, {}, only='invalid handle')


def test_every_entry_has_three_double_faults():
    for entry in P.PARAMS:
        rows = [r for t, rs in P.CASES.items() if t.split(' ')[0] == entry for r in rs]
        for form in 'hd':
            assert sum(1 for what, forms, *_ in rows if ' + ' in what and form in forms) >= 3, (entry, form)


# ---- Python side -----------------------------------------------------------------------------------------------------------

ROWS = {
    'rows past the end': 'rows (0, 4) is not a range within the 3 rows',
    'rows negative': 'rows (-1, 2) is not a range within the 3 rows',
    'rows reversed': 'rows (2, 1) is not a range within the 3 rows',
    'rows not a pair': 'rows must be (begin, end), not (1,)',
    'rows not integers': 'rows must be two integers, not (0.0, 2.0)',
}
SDDMM = {
    'U rows': 'U has 2 rows, expected 3',
    'V rows': 'V has 5 rows, expected 4',
    'k mismatch': 'U and V have 5 and 6 columns',
    'mixed f32/f64': 'U and V must have the same dtype, not float32 and float64',
    '1-D panel': 'panels must be 2-D, not of shapes (3,) and (4, 5)',
    'k = 0': 'panels have no columns (k = 0)',
}
GRAM = dict(ROWS, **{
    'V rows': 'V has 5 rows, expected 4',
    '1-D V': 'V must be 2-D, not of shape (4,)',
    'k = 0': 'V has no columns (k = 0)',
    'integer V': 'V must be float32 or float64, not int64',
    'float16 V': 'V must be float32 or float64, not float16',
    'base shape': 'base must be float64 of shape (5, 5), not float64 of shape (5, 4)',
    'base 1-D': 'base must be float64 of shape (5, 5), not float64 of shape (25,)',
    'base dtype': 'base must be float64 of shape (5, 5), not float32 of shape (5, 5)',
})
RHS = "rhs must be one of ['one_plus_values', 'ones', 'values'], not "
RIDGE = 'the per-entry ridge must be one real number, not '
ALS = dict(GRAM, **{
    'rhs unknown': RHS + "'value'",
    'rhs a code': RHS + '1',
    'rhs None': RHS + 'None',
    'ridge per row': RIDGE + 'array([1., 1., 1.])',
    'ridge a string': RIDGE + "'0.1'",
    'ridge None': RIDGE + 'None',
    'ridge complex': RIDGE + '1j',
})
PAIR = {
    'U rows': 'U has 4 rows, expected 3',
    'V rows': 'V has 5 rows, expected 4',
    '1-D U': 'panels must be 2-D, not of shapes (3,) and (4, 5)',
    '1-D V': 'panels must be 2-D, not of shapes (3, 5) and (4,)',
    'k differs': 'U and V have 5 and 4 columns',
    'k = 0': 'panels have no columns (k = 0)',
    'mixed dtypes': 'U and V must have the same dtype, not float64 and float32',
    'integer panels': 'U and V must be float32 or float64, not int64',
    'float16 panels': 'U and V must be float32 or float64, not float16',
}
TOPK_SCORES = dict(ROWS, **PAIR, **{
    'n = 0': 'n must be at least 1, not 0',
    'n negative': 'n must be at least 1, not -3',
    'n a float': 'n must be an integer, not 2.0',
    'n a bool': 'n must be an integer, not True',
    'n None': 'n must be an integer, not None',
    'min_score NaN': 'min_score is NaN',
    'min_score a string': "min_score must be one real number or None, not '0'",
    'min_score per row': 'min_score must be one real number or None, not array([0., 0., 0.])',
})
RANK_ENTRIES = dict(ROWS, **PAIR, **{
    'test of more columns': 'seen is 3 x 4 but test is 3 x 5',
    'test of fewer rows': 'seen is 3 x 4 but test is 2 x 4',
    'test an array': 'test must be a CSR or a handle, not ndarray',
    'test None': 'test must be a CSR or a handle, not NoneType',
})


def _raises(text, fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    assert str(ei.value) == text


def _no_library(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_sddmm', 'csrk_gram_rows', 'csrk_als_rows', 'csrk_topk_scores', 'csrk_rank_entries', 'csrk_create', 'csrk_row_extent'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K, K.hip_h(12345, 3, 4, 4)


def test_the_tables_are_those_of_the_host_tests():
    assert set(SDDMM) == set(test_sddmm_host._bad_cases()) and set(GRAM) == set(test_gram_host._bad_cases())
    assert set(ALS) == set(test_als_host._bad_als()) and set(TOPK_SCORES) == set(test_topk_scores_host._bad())
    assert set(RANK_ENTRIES) == set(test_rank_entries_host._bad())


@pytest.mark.parametrize('case', sorted(SDDMM))
def test_sddmm_words(case, monkeypatch):
    K, h = _no_library(monkeypatch)
    _raises(SDDMM[case], K.sddmm, h, *test_sddmm_host._bad_cases()[case])


@pytest.mark.parametrize('case', sorted(GRAM))
def test_gram_words(case, monkeypatch):
    K, h = _no_library(monkeypatch)
    kw = test_gram_host._bad_cases()[case]
    _raises(GRAM[case], K.gram_args, h, kw['V'], kw.get('rows'), kw.get('base'))
    _raises(GRAM[case], K.gram_rows, h, kw['V'], False, kw.get('rows'), kw.get('base'))


@pytest.mark.parametrize('case', sorted(ALS))
def test_als_words(case, monkeypatch):
    K, h = _no_library(monkeypatch)
    kw = test_als_host._bad_als()[case]
    args = (kw.get('rhs', 'values'), kw.get('base'), kw.get('reg', 0.0), kw.get('rows'))
    _raises(ALS[case], K.als_args, h, kw['V'], *args)
    _raises(ALS[case], K.als_rows, h, kw['V'], False, *args)


@pytest.mark.parametrize('case', sorted(TOPK_SCORES))
def test_topk_scores_words(case, monkeypatch):
    K, h = _no_library(monkeypatch)
    kw = test_topk_scores_host._bad()[case]
    args = (kw['U'], kw['V'], kw.get('n', 2), kw.get('min_score'), kw.get('rows'))
    _raises(TOPK_SCORES[case], K.topk_scores_args, h, *args)
    _raises(TOPK_SCORES[case], K.topk_scores, h, *args)
    if case not in ('U rows', 'V rows', 'rows past the end'):          # without a handle the panels give the shape
        _raises(TOPK_SCORES[case], K.topk_scores_args, None, *args)


@pytest.mark.parametrize('case', sorted(RANK_ENTRIES))
def test_rank_entries_words(case, monkeypatch):
    K, seen_h = _no_library(monkeypatch)
    kw = test_rank_entries_host._bad()[case]
    test = kw.get('test', (3, 4))
    test_h = K.hip_h(777, test[0], test[1], 3) if isinstance(test, tuple) else test
    _raises(RANK_ENTRIES[case], K.rank_entries_args, seen_h, test_h, kw['U'], kw['V'], kw.get('rows'))
    _raises(RANK_ENTRIES[case], K.rank_entries, seen_h, test_h, kw['U'], kw['V'], kw.get('rows'))


def test_requests_wrong_in_two_ways_keep_their_order(monkeypatch):
    K, h = _no_library(monkeypatch)
    U, V, V4 = np.ones((3, 5)), np.ones((4, 5)), np.ones((4, 4))
    Ui, Vi4 = U.astype(np.int64), V4.astype(np.int64)
    mixed = 'U and V must have the same dtype, not float64 and float32'
    # two panels: 2-D, then one dtype, then (topk_scores, rank_entries: a panel dtype, then) one k, then k >= 1, then the rows
    for fn, args in ((K.sddmm, ()), (K.topk_scores_args, (2,)), (K.rank_entries_args, ())):
        pre = (h, h) if fn is K.rank_entries_args else (h,)
        _raises(mixed, fn, *pre, U, V4.astype(np.float32), *args)                                   # mixed dtypes + different k
        _raises('panels must be 2-D, not of shapes (3,) and (4, 4)', fn, *pre, np.ones(3, np.float32), V4, *args)
        _raises('U and V have 5 and 4 columns', fn, *pre, np.ones((2, 5)), V4, *args)               # different k + U's rows
        _raises('panels have no columns (k = 0)', fn, *pre, np.ones((2, 0)), np.ones((4, 0)), *args)
    _raises('U and V have 5 and 4 columns', K.sddmm, h, Ui, Vi4)                                     # integer panels + different k:
    _raises('U must be float32 or float64, not int64', K.sddmm, h, Ui, V.astype(np.int64))         # sddmm leaves the dtype to _panel
    _raises('U and V must be float32 or float64, not int64', K.topk_scores_args, h, Ui, Vi4, 2)
    _raises('U and V must be float32 or float64, not int64', K.rank_entries_args, h, h, Ui, Vi4)
    # topk_scores: panels, n, min_score, rows
    _raises('n must be at least 1, not 0', K.topk_scores_args, h, U, V, 0, None, (1,))              # rows not a pair + n = 0
    _raises('U has 2 rows, expected 3', K.topk_scores_args, h, np.ones((2, 5)), V, 0)
    _raises('n must be an integer, not 2.5', K.topk_scores_args, h, U, V, 2.5, float('nan'))
    _raises('min_score is NaN', K.topk_scores_args, h, U, V, 2, float('nan'), (2, 1))
    _raises('rows must be (begin, end), not 5', K.topk_scores_args, h, U, V, 2, None, 5)
    _raises('rows must be two integers, not (True, 9)', K.topk_scores_args, h, U, V, 2, None, (True, 9))
    # rank_entries: the handles, then topk_scores' panels and rows
    _raises('test must be a CSR or a handle, not NoneType', K.rank_entries_args, h, None, np.ones(3), V)
    _raises('seen is 3 x 4 but test is 3 x 5', K.rank_entries_args, h, K.hip_h(777, 3, 5, 3), U, V4)
    # gram: V (2-D, dtype, k, rows of V), rows, base; als adds rhs, then the ridge
    Vb = np.ones((5, 0), np.int64)
    _raises('V must be float32 or float64, not int64', K.gram_args, h, Vb, (1,), np.ones(3))        # dtype + k = 0 + V's rows + ...
    _raises('V has no columns (k = 0)', K.gram_args, h, np.ones((5, 0)), (1,))
    _raises('V has 5 rows, expected 4', K.gram_args, h, np.ones((5, 5)), (1,))
    _raises('rows must be (begin, end), not (1,)', K.gram_args, h, V, (1,), np.ones(3))
    _raises('rows must be two integers, not (0, False)', K.gram_args, h, V, (0, False), np.ones(3))
    _raises('rows (2, 1) is not a range within the 3 rows', K.als_args, h, V, 'value', np.ones(3), None, (2, 1))
    _raises('base must be float64 of shape (5, 5), not float64 of shape (3,)', K.als_args, h, V, 'value', np.ones(3), None)
    _raises(RHS + "'value'", K.als_args, h, V, 'value', None, None)
    _raises(RIDGE + 'True', K.als_args, h, V, 'ones', None, True)
