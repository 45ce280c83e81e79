"""
The SpMV light stream (spmv_lstream_kernel, its plan builders and the copy pass ls_stage_kernel) on the cases of
tests/lstream_cases.py, every one of them in three forms: the stream without a pack (CSRK_SPMV_HOT=0), with the pack
(CSRK_SPMV_HOT=1, CSRK_LS_STAGE=0) and with the pack and cold staging (CSRK_LS_STAGE=1), always with CSRK_SPMV_STREAM=1, the
merge algorithm, and the long-row split forced where the case has cut rows (off otherwise).  Per case and form, on each of
three products into a y filled with NaN:
  1. csrk_spmv_plan_stats equals the module's model of the layout field by field, and csrk_spmv_cut_rows the model's cut set;
  2. every row meets 1e-12 * sum |a_ij x_j| against the oracle's sequential loop (the bar of tests/test_gpu_spmv.py; rows
     stay at or below 4096 entries, so 4096 * 2^-53 lies under it), nothing is NaN, rows without an entry hold +0.0;
  3. every row that the model places inside one tile and whose sum is stored at most LS_SEQ = 3 lanes after the lane it starts
     in (Layout.exact_rows: every row of at most 24 entries but the matrix's last, rows of 25 unless they start in a lane's last
     slot, some of up to 31) equals the sequential loop BIT FOR BIT, in every form: the kernel hands such a run's sum on in the
     reference's own order.  (As first worded -- every row of at most 25 entries inside a tile -- the claim did not hold: a
     25-entry row from a lane's last slot is stored by a fifth lane, and the last tile's padding continues the last row.)
Three representative cases also run with float32 and with no values, int64 row pointers, a float32 x (float32 products
where the values are float32 too) and through the two-part entry.  The forms of one case give the same bits as each other
(the pack and staging only change where an x value is read from), the two-part product equals the whole, and with x and y
as views at element offset 1 of NaN-filled buffers nothing outside y is written and no NaN reaches y.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import lstream_cases as S

pytestmark = pytest.mark.gpu

ALL = S.names()
VARIANTS = ('f4', 'none', 'ptr64', 'f32x', 'f4f32x', 'part')
_RUNS, _REFS = {}, {}


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _typed(name, variant):
    "(matrix, x) of a variant: the case's own float64 arrays retyped"
    c = S.build(name, _cus())
    m = c.m.retyped(vals={'f4': 'f4', 'f4f32x': 'f4', 'none': 'none'}.get(variant, 'f8'), ptr64=variant == 'ptr64')
    return c, m, (c.x.astype(np.float32) if variant in ('f32x', 'f4f32x') else c.x)


def _ref(name, variant):
    "(oracle's product, sum |a_ij x_j| per row): computed once per case and variant"
    key = (name, 'f8' if variant in ('ptr64', 'part') else variant)
    if key not in _REFS:
        from oracle import oracle as O
        _, m, x = _typed(name, key[1])
        ref = O.mult_vec(m.nrows, m.ncols, m.rowptrs, m.colinds, m.values, x)
        bound = O.mult_vec(m.nrows, m.ncols, m.rowptrs, m.colinds, None if m.values is None else np.abs(m.values), np.abs(x))
        ref.flags.writeable = bound.flags.writeable = False
        _REFS[key] = (ref, bound)
    return _REFS[key]


def _run(name, form, variant='f8', offset=0):
    """
    Three products of (case, form, variant) on a fresh handle, each into a NaN-filled buffer with `offset` spare elements on
    either side of x and y: the three buffers, the plan's census and its cut rows (memoised: several tests read one run).
    """
    key = (name, form, variant, offset)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from csr_amd import CSR
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    c, m, x = _typed(name, variant)
    dev = torch.device('cuda', 0)
    nan = float('nan')
    with _environ(dict(S.env_of(c, form), CSRK_HANDLE_CACHE='0')):
        h = K.to_handle(CSR(m.nrows, m.ncols, m.nnz, m.rowptrs, m.colinds, m.values, _cast=False))
        try:
            K.set_spmv_algo(h, 'merge')
            xb = torch.full((m.ncols + 2 * offset,), nan, dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device=dev)
            xv = xb[offset:offset + m.ncols]
            xv.copy_(torch.tensor(x))      # (a copy: the case's arrays are read-only)
            yb = torch.empty(m.nrows + 2 * offset, dtype=torch.float64, device=dev)
            yv = yb[offset:offset + m.nrows]
            out, after1 = [], None
            for _ in range(3):
                yb.fill_(nan)
                if variant == 'part':
                    check(lib.csrk_spmv_device_part(h.H, xv.data_ptr(), yv.data_ptr(), None, 1))
                    torch.cuda.synchronize()
                    after1 = yb.cpu().numpy()
                    check(lib.csrk_spmv_device_part(h.H, xv.data_ptr(), yv.data_ptr(), None, 2))
                elif x.dtype == np.float32:
                    check(lib.csrk_spmv_f32x_device(h.H, xv.data_ptr(), yv.data_ptr(), None))
                else:
                    check(lib.csrk_spmv_device(h.H, xv.data_ptr(), yv.data_ptr(), None))
                torch.cuda.synchronize()
                out.append(yb.cpu().numpy())
            stats = K.spmv_plan_stats(h)
            n = C.c_int64(0)
            check(lib.csrk_spmv_cut_rows(h.H, None, 0, C.byref(n)))
            rows = torch.zeros(max(n.value, 1), dtype=torch.int32, device=dev)
            if n.value:
                check(lib.csrk_spmv_cut_rows(h.H, rows.data_ptr(), n.value, C.byref(n)))
            cut = rows.cpu().numpy()[:n.value].astype(np.int64)
        finally:
            K.release_handle(h)
    _RUNS[key] = dict(buffers=out, after1=after1, stats=stats, cut=cut, algo='merge')
    return _RUNS[key]


def _check_census(c, form, variant, r):
    a = c.layout(form, _cus())
    want = a.census(f32=variant in ('f4', 'f4f32x'))
    got = {k: r['stats'][k] for k in want}
    assert got == want, (c.name, form, variant, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    assert np.array_equal(r['cut'], a.cut), (c.name, form, r['cut'][:8], a.cut[:8])
    return a


def _check_product(c, a, variant, y, what):
    "checks 2 and 3 of the module docstring on one product"
    ref, bound = _ref(c.name, variant)
    assert y.shape == ref.shape and not np.isnan(y).any(), (what, np.flatnonzero(np.isnan(y))[:8])
    err = np.abs(y - ref)
    bad = np.flatnonzero(~(err <= 1e-12 * bound + 1e-300))
    assert bad.size == 0, (what, bad[:8], y[bad[:8]], ref[bad[:8]])
    empty = np.flatnonzero(np.diff(np.asarray(c.m.rowptrs, dtype=np.int64)) == 0)
    assert np.all(y[empty].view(np.int64) == 0), (what, 'rows without an entry must hold +0.0')
    rows = a.exact_rows()
    diff = rows[y[rows].view(np.int64) != ref[rows].view(np.int64)]
    assert diff.size == 0, (what, 'rows the in-order hand-over reaches differ from the sequential loop', diff[:8],
                            a.view_lens[diff[:8]], (a.first[diff[:8]] % S.TILE), y[diff[:8]], ref[diff[:8]])


def _check_run(name, form, variant='f8'):
    c = S.build(name, _cus())
    assert not S.failed_preconditions(c, _cus()), S.failed_preconditions(c, _cus())      # on THIS device's CU count
    r = _run(name, form, variant)
    a = _check_census(c, form, variant, r)
    for i, y in enumerate(r['buffers']):
        _check_product(c, a, variant, y, (name, form, variant, f'product {i}'))
        assert np.array_equal(y.view(np.int64), r['buffers'][0].view(np.int64)), (name, form, variant, i)
    return c, a, r


@pytest.mark.parametrize('form', S.FORMS)
@pytest.mark.parametrize('name', ALL)
def test_case_in_every_form(name, form):
    _check_run(name, form)


@pytest.mark.parametrize('name', ALL)
def test_forms_reach_their_kernels(name):
    "the censuses of the three forms show the three modes the default build can reach, wherever the case can be staged"
    c = S.build(name, _cus())
    st = {f: _run(name, f)['stats'] for f in S.FORMS}
    assert all(s['stream'] == 1 for s in st.values())
    assert st['nopack']['n_hot'] == 0 and st['nopack']['ls_staged'] == 0 and st['nopack']['ls_idx24'] == 0
    assert st['pack']['ls_staged'] == 0 and st['pack']['ls_idx24'] == 0 and st['pack']['ls_stage_blocks'] == 0
    if [c.layout(f, _cus()).mode() for f in S.FORMS] == ['LS_PLAIN', 'LS_PLAIN+pack', 'LS_RND24']:
        assert st['pack']['n_hot'] > 0 and st['staged']['n_hot'] == st['pack']['n_hot']
        assert st['staged']['ls_staged'] > 0 and st['staged']['ls_idx24'] == 1 and st['staged']['ls_round_tiles'] >= S.NW
        assert st['staged']['ls_stage_blocks'] * st['staged']['ls_stage_width'] >= c.m.ncols
    else:
        assert name in ('nview-1', 'nview-2', 'ncols-1') and st['staged']['ls_staged'] == 0


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('form', S.FORMS)
@pytest.mark.parametrize('name', S.REPRESENTATIVE)
def test_value_index_and_vector_types(name, form, variant):
    c, a, r = _check_run(name, form, variant)
    base = _run(name, form)['buffers'][2]
    y = r['buffers'][2]
    if variant in ('ptr64', 'part'):            # the same numbers through other pointers / in two parts: the same bits
        assert np.array_equal(y.view(np.int64), base.view(np.int64))
    if variant == 'part':                       # after part 1 the cut rows hold 0.0 and every other row is final
        keep = np.ones(c.m.nrows, dtype=bool)
        keep[a.cut] = False
        assert np.all(r['after1'][a.cut].view(np.int64) == 0)
        assert np.array_equal(r['after1'][keep].view(np.int64), base[keep].view(np.int64))
    if variant == 'f4f32x':                     # float32 products, not the float64 ones
        assert np.max(np.abs(_ref(name, 'f4f32x')[0] - _ref(name, 'f4')[0])) > 1e-10


@pytest.mark.parametrize('name', ('pack-8177', 'pack-15361', 'long-rows', 'gaps', 'long-cut200'))
def test_forms_agree_bit_for_bit(name):
    "the pack and staging only change where an x value is read from"
    ys = [_run(name, f)['buffers'][2] for f in S.FORMS]
    assert np.array_equal(ys[0].view(np.int64), ys[1].view(np.int64)) and np.array_equal(ys[0].view(np.int64), ys[2].view(np.int64))


@pytest.mark.parametrize('form,name', [('nopack', 'gaps'), ('pack', 'pack-15361'), ('staged', 'stage-batch-8193'), ('staged', 'starts-512-rowid')])
def test_nothing_outside_y_is_written(form, name):
    "x and y as views at element offset 1 of NaN-filled buffers: the same bits as on aligned buffers, the guard elements untouched"
    c = S.build(name, _cus())
    aligned, shifted = _run(name, form), _run(name, form, offset=1)
    a = _check_census(c, form, 'f8', shifted)
    for i, (ya, yb) in enumerate(zip(aligned['buffers'], shifted['buffers'])):
        assert np.isnan(yb[0]) and np.isnan(yb[-1]), (name, form, i)
        assert not np.isnan(yb[1:-1]).any(), (name, form, i)
        assert np.array_equal(ya.view(np.int64), yb[1:-1].view(np.int64)), (name, form, i)
        _check_product(c, a, 'f8', yb[1:-1], (name, form, 'offset 1', i))


def test_union_of_censuses():
    "both layouts, the plain and the 3-byte-staged modes, float32 and float64 streams, pack slots below and above the LDS limits, two rounds in a workgroup"
    seen = set()
    for name in ALL:
        for f in S.FORMS:
            s = _run(name, f)['stats']
            seen.add('dense' if s['ls_dense'] else 'row ids')
            seen.add('staged, 3-byte words' if s['ls_idx24'] else 'plain with a pack' if s['n_hot'] else 'plain')
            assert not (s['ls_staged'] and not s['ls_idx24'])                      # LS_RND with 4-byte words: not in the default build
            if s['n_hot']:
                seen.add(('pack within LDS' if s['n_hot'] == s['ls_hot_lds'] else 'pack beyond LDS') + (', staged' if s['ls_staged'] else ''))
            if s['ls_wg_rounds'] >= 2:
                seen.add('two rounds in a workgroup' + (', staged' if s['ls_staged'] else ''))
    seen.add('float32 stream' if _run('gaps', 'staged', 'f4')['stats']['ls_f32'] else 'float64 stream')
    seen.add('float32 stream' if _run('gaps', 'staged')['stats']['ls_f32'] else 'float64 stream')
    want = {'dense', 'row ids', 'plain', 'plain with a pack', 'staged, 3-byte words', 'pack within LDS', 'pack beyond LDS',
            'pack within LDS, staged', 'pack beyond LDS, staged', 'two rounds in a workgroup', 'two rounds in a workgroup, staged',
            'float32 stream', 'float64 stream'}
    assert want <= seen, sorted(want - seen)
