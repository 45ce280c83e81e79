"""
The long-row class of csrk_als_rows_cg (include/csrk.h, rule C11) on the host side, without a GPU: its three kinds of entry
(the switch, the limits, the census) are declared, exported, in the ctypes table and addressable; the limits are sane and
need no device; the switch round-trips, refuses what is below -1 and follows CSRK_ALS_CG_LONG (checked in a fresh child
process); the census is all 0 after a refused call.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_als_cg_set_long', 'csrk_als_cg_get_long', 'csrk_als_cg_long_limits', 'csrk_als_cg_last_stats')


@pytest.fixture
def restore():
    "the process-wide switch goes back to following the environment"
    from csr_amd.kernels import hip as K
    try:
        yield K
    finally:
        K.als_cg_set_long(None)


def test_entries_declared_exported_and_in_the_table():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    from csr_amd.kernels import raw
    for name in NAMES:
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert raw.address(name)
    # rule C11 is written down, and the older entries keep their shape
    assert 'C11.' in open(os.path.join(ROOT, 'include', 'csrk.h')).read()
    from csr_amd.kernels import hip as K
    assert len(K.als_cg_limits()) == 3


def test_limits_are_sane_and_need_no_device():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID
    lim = K.als_cg_long_limits()
    assert len(lim) == 8
    L, threads, S, c = lim[0], lim[1], lim[2], lim[3:7]
    assert L >= 1 and L in (1024, 2048, 4096, 8192, 16384)
    assert threads >= 64 and threads % 64 == 0 and S >= 1 and S % threads == 0
    assert all(x >= 2 for x in c) and lim[7] == 2
    # the image fits one workgroup's LDS: buffers x C x (row bytes) for each class
    for C_, rowbytes in zip(c, (64 * 8, 128 * 8, 64 * 4, 128 * 4)):
        assert lim[7] * C_ * rowbytes <= 160 * 1024
    # n = 1 writes one slot; NULL is refused
    two = (ctypes.c_int64 * 2)(-5, -5)
    assert lib.csrk_als_cg_long_limits(two, 1) == 0 and two[0] == L and two[1] == -5
    assert lib.csrk_als_cg_long_limits(None, 1) == ERR_INVALID
    assert lib.csrk_als_cg_last_stats(None, 1) == ERR_INVALID
    assert lib.csrk_als_cg_get_long(None) == ERR_INVALID
    st = (ctypes.c_int64 * 2)(-5, -5)
    assert lib.csrk_als_cg_last_stats(st, 1) == 0 and st[1] == -5


def test_switch_round_trips_and_refuses(restore):
    K = restore
    from csr_amd._lib import lib, ERR_INVALID
    for v in (0, 1, 2 ** 31, 701):
        K.als_cg_set_long(v)
        assert K.als_cg_get_long() == v
    assert lib.csrk_als_cg_set_long(-2) == ERR_INVALID and lib.csrk_last_error()
    assert K.als_cg_get_long() == 701                        # a refused setting changes nothing
    for bad in (-2, 1.5, '7', True):
        with pytest.raises(ValueError):
            K.als_cg_set_long(bad)
    assert K.als_cg_get_long() == 701
    K.als_cg_set_long(None)                                  # back to the environment: here the default, unless the variable is set
    if not os.environ.get('CSRK_ALS_CG_LONG'):
        assert K.als_cg_get_long() == K.als_cg_long_limits()[0]


def _child(env_value, code):
    env = dict(os.environ)
    env.pop('CSRK_ALS_CG_LONG', None)
    if env_value is not None:
        env['CSRK_ALS_CG_LONG'] = env_value
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.split()


def test_minus_one_follows_the_environment():
    "in fresh child processes: the variable's count, 0 = off, unset or not a count = the default; a set value wins until -1"
    code = ('from csr_amd.kernels import hip as K\n'
            'print(K.als_cg_get_long())\n'
            'K.als_cg_set_long(9)\n'
            'print(K.als_cg_get_long())\n'
            'K.als_cg_set_long(-1)\n'
            'print(K.als_cg_get_long(), K.als_cg_long_limits()[0])\n')
    for value, want in (('12345', 12345), ('0', 0), ('1', 1), (None, None), ('', None), ('many', None), ('-4', None), ('12x', None)):
        first, nine, again, default = (int(x) for x in _child(value, code))
        want = default if want is None else want
        assert (first, nine, again) == (want, 9, want), value


def test_last_stats_is_all_zero_after_a_refused_call(restore):
    K = restore
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64, ALS_RHS_VALUES
    V, out = np.ones((4, 2)), np.full(6, 7.0)
    K.als_cg_set_long(3)
    for H, steps in ((0, 3), (12345, 3), (0, -1)):           # a null handle, a stale one, a scalar refusal
        assert lib.csrk_als_rows_cg(H, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, steps, 0.0, None, 2,
                                    out.ctypes.data, 2, None, None) == ERR_INVALID
        assert K.als_cg_last_stats() == (0,) * 6
        assert lib.csrk_als_rows_cg_device(H, 0, 3, None, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, steps, 0.0, None, 2, None, 2,
                                           None, None, None) == ERR_INVALID
        assert K.als_cg_last_stats() == (0,) * 6
    assert np.all(out == 7.0)
