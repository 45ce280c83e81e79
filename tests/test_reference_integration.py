"""
INTEGRATION.md section 1, executed without the reference: the `hip` kernel module is registered as an out-of-tree
module through the public registry dict (csr_amd.kernels mirrors csr/kernels/__init__.py:7-123), and a caller that
knows nothing of csr_amd drives it the way the reference's CSR.mult_vec / CSR.multiply do (csr/csr.py:543-567,
580-590): get_kernel(), to_handle on a plain object with only the fields of the reference's struct (csr/csr.py:79-100),
the product, release_handle.  Runs in a subprocess.  Without a GPU the call must reach libcsrk and fail loudly there
(CsrkError from csrk_create), which proves the routing; with a GPU it must produce the product.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import sys, types, numpy as np
sys.dont_write_bytecode = True
import csr_amd.kernels as KS
import csr_amd.kernels.hip as hip
from csr_amd._lib import CsrkError


def foreign_csr(nrows, ncols, rowptrs, colinds, values):
    "the reference's CSR as the kernel protocol sees it: nrows / ncols / nnz / rowptrs / colinds / values, nothing else"
    return types.SimpleNamespace(nrows=nrows, ncols=ncols, nnz=len(colinds), rowptrs=np.asarray(rowptrs, np.int32),
                                 colinds=np.asarray(colinds, np.int32), values=values)


KS.kernels['hip_plugin'] = hip
A = foreign_csr(4, 3, [0, 2, 3, 3, 4], [1, 2, 0, 1], np.arange(4.0))
At = foreign_csr(3, 4, [0, 1, 3, 4], [1, 0, 3, 0], np.array([2.0, 0.0, 3.0, 1.0]))
with KS.use_kernel('hip_plugin'):
    K = KS.get_kernel()
    assert K is hip
    try:
        with KS.releasing(K.to_handle(A), K) as h:
            y = K.mult_vec(h, np.ones(3))
        assert list(y) == [1.0, 2.0, 0.0, 3.0], y
        with KS.releasing(K.to_handle(A), K) as ha, KS.releasing(K.to_handle(At), K) as hb, \
                KS.releasing(K.mult_ab(ha, hb), K) as hp:
            P = K.from_handle(hp)
        assert sorted(v for v in np.asarray(P.values).tolist() if v != 0.0) == [1.0, 4.0, 9.0]
        print('COMPUTED')
    except CsrkError as e:
        assert 'hip' in str(e).lower()
        print('ROUTED')
'''


def test_hip_kernel_registers_through_the_plugin_registry(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1', PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-c', SCRIPT], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] in ('ROUTED', 'COMPUTED')
