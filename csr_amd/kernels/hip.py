"""
The `hip` kernel: the reference's kernel-module protocol (csr/kernel.py:9-16,
docs/kernels.rst:61-104) implemented on libcsrk.so -- hand-written HIP kernels for
MI355X (gfx950) behind the C ABI of include/csrk.h.

Protocol members (same names and meaning as csr/kernels/numba/__init__.py:13-67 and
csr/kernels/mkl/*): max_nnz, to_handle, from_handle, release_handle, order_columns,
mult_ab, mult_abt, mult_vec.  Extra members for the operations the reference runs
outside its kernel protocol but on the same hot path: transpose, row_nnzs, unit_rows,
center_rows, filter_zeros, pick_rows, mult_dense, sddmm, gram_rows, als_rows, als_rows_cg, solve_blocks, topk_rows, combine, coalesce,
is_canonical, topk_scores, topk_scores_for, rank_entries, rank_entries_for, knn_scores, knn_reach_index.

A handle owns a copy of the matrix in HBM, like the MKL kernel's handle
(csr/kernels/mkl/handle.py:47-70).  There is no CPU fallback: without a GPU every call
raises csr_amd._lib.CsrkError.

Handle cache.  The reference's callers make a handle per operation (CSR.mult_vec: to_handle -> mult_vec ->
release_handle, csr/csr.py:580-583); for a matrix in HBM that is a PCIe copy of the whole matrix per product, and
libcsrk's planned kernels (built on a handle's second product) are never reached.  docs/kernels.rst:69-80 lets a
kernel copy in to_handle and obliges the caller to release explicitly, so `to_handle` here keeps the device copy of
a released handle alive and hands it out again when the SAME CSR object comes back with the SAME arrays -- but only
where a stale copy cannot go unseen:
  * by default only for CSR classes that declare `__csrk_cacheable__ = True` (csr_amd.CSR does): their own mutators
    call `invalidate`, their arrays own their memory, and WHILE A DEVICE COPY IS CACHED THE THREE HOST ARRAYS ARE
    WRITE-PROTECTED (ndarray.flags.writeable = False; restored when the copy is dropped) -- `A.values[i] = v` between
    two products raises "assignment destination is read-only" instead of multiplying by the old matrix.  Call
    `invalidate(A)` first (it drops the copy and restores the flags), then edit.  (NumPy raises that error itself:
    the message cannot name `invalidate`; INTEGRATION.md section 2a does.)  The reference's numba handle
    aliases the host arrays (csr/kernels/numba/__init__.py:16-27), so there an edit is simply seen; here it is
    either seen or refused, never missed.  (A view of an array taken BEFORE its first product keeps its own
    writeable flag -- the one alias the guard cannot reach; the sampled fingerprint below is the second line.)
  * CSRK_HANDLE_CACHE=1 extends the cache to every CSR class WITHOUT the write guard (fingerprint only: a single
    element poked into a foreign class's arrays is not seen -- for callers who never edit in place);
    CSRK_HANDLE_CACHE=0 turns it off: every to_handle copies, like the MKL kernel (csr/kernels/mkl/handle.py:61-70);
  * key: id(csr) + shape + nnz + the three arrays' data pointers and dtypes; the entry dies with the CSR object
    (weakref.finalize), so a recycled id or address can never hit; a sampled fingerprint of the arrays (first / last
    32 + 2048 strided elements each) is compared on every hit;
  * a cached copy is handed out only while IDLE: a second live handle on the same CSR gets a copy of its own, so the
    in-place protocol operations (order_columns, unit_rows, center_rows), which also detach their handle from the
    cache, never change a device copy another live handle is reading;
  * idle device copies are evicted least-recently-used beyond CSRK_HANDLE_CACHE_BYTES (default 16 GiB; a copy
    counts with its SpMV / SpMM plans) and whenever a library call runs out of device memory (retried once).
"""
import ctypes as C
import numbers
import os
import collections
import threading
import weakref

import numpy as np

from .. import _lib
from .._lib import lib, check, ptr, handle_t

# int64 row pointers are supported on the device, so the limit is HBM, not the index type
# (numba kernel: i8.max, csr/kernels/numba/__init__.py:13; MKL: i4.max, mkl/__init__.py:5)
max_nnz = np.iinfo('i8').max

_VAL_CODES = {None: _lib.VAL_NONE, np.dtype('f4'): _lib.VAL_F32, np.dtype('f8'): _lib.VAL_F64}


class hip_h:
    "Opaque handle (cf. mkl_h, csr/kernels/mkl/handle.py:30-43): H is the csrk_handle_t."
    __slots__ = ('H', 'nrows', 'ncols', 'nnz', 'csr_ref', '_entry')

    def __init__(self, H, nrows, ncols, nnz, csr_ref=None):
        self.H = H
        self.nrows = nrows
        self.ncols = ncols
        self.nnz = nnz
        self.csr_ref = csr_ref
        self._entry = None          # the handle cache's record when the device copy is shared (module docstring)

    def __repr__(self):
        return f'<hip_h {self.nrows}x{self.ncols} ({self.nnz} nnz) H={self.H:#x}>'


def _live(h):
    if not h.H:
        raise ValueError('handle has been released')
    return h.H


# ---- handle cache ------------------------------------------------------------------------------------------
class _Entry:
    __slots__ = ('H', 'refs', 'bytes', 'key', 'finger', 'tick', 'cached', 'fin', 'guard')


_cache_lock = threading.RLock()
_cache = {}                     # key -> _Entry (live or idle device copies that may be handed out again)
_guards = {}                    # id(array) -> [array, entries guarding it]: host arrays write-protected while cached
_tick = 0
_SAMPLE = 2048


def _cache_mode():
    "'off' | 'guarded' (classes that declare __csrk_cacheable__, write-protected arrays) | 'all' (fingerprint only)"
    v = os.environ.get('CSRK_HANDLE_CACHE')
    if v is None or v == '':
        return 'guarded'
    return 'off' if v in ('0', 'off', 'false') else 'all'


def _cache_budget():
    return int(os.environ.get('CSRK_HANDLE_CACHE_BYTES', str(16 << 30)))


def _arr_key(a):
    return (0, '') if a is None else (a.ctypes.data, a.dtype.str)


def _sample(a):
    if a is None or a.size == 0:
        return b''
    n = a.size
    if n <= 4 * _SAMPLE:
        return a.tobytes()
    step = n // _SAMPLE
    return a[:32].tobytes() + a[::step].tobytes() + a[-32:].tobytes()


def _fingerprint(rps, cis, vs):
    return hash((_sample(rps), _sample(cis), _sample(vs)))


def _protect(arrays):
    "write-protect the host arrays of a cached copy (caller holds the lock); returns what to hand to _unprotect"
    held = []
    for a in arrays:
        if a is None:
            continue
        g = _guards.get(id(a))
        if g is not None and g[0] is a:
            g[1] += 1                    # already guarded for another cached copy that shares it (CSR.copy(copy_structure=False))
            held.append(a)
            continue
        if not a.flags.writeable:        # read-only before we came: not ours to restore
            continue
        _guards[id(a)] = [a, 1]
        a.flags.writeable = False
        held.append(a)
    return held


def _unprotect(held):
    for a in held:
        g = _guards.get(id(a))
        if g is None:
            continue
        g[1] -= 1
        if g[1] <= 0:
            del _guards[id(a)]
            a.flags.writeable = True


def _drop_entry(e):
    "remove from the index; free the device copy once nobody holds it (caller holds the lock)"
    if e.cached:
        e.cached = False
        if _cache.get(e.key) is e:
            del _cache[e.key]
    if e.guard:
        held, e.guard = e.guard, None
        _unprotect(held)
    if e.refs == 0 and e.H:
        H, e.H = e.H, 0
        check(lib.csrk_free(H))


def _on_csr_collected(key):
    with _cache_lock:
        e = _cache.get(key)
        if e is not None:
            _drop_entry(e)


def _evict_idle(budget):
    "free idle cached copies, least recently used first, until the idle ones fit `budget` bytes"
    with _cache_lock:
        idle = sorted((e for e in _cache.values() if e.refs == 0), key=lambda e: e.tick)
        total = sum(e.bytes for e in idle)
        for e in idle:
            if total <= budget:
                break
            total -= e.bytes
            _drop_entry(e)


def flush_handle_cache():
    "free every idle cached device copy (live handles are untouched)"
    _evict_idle(0)


def invalidate(csr):
    """
    Forget the cached device copy of `csr` and make its arrays writable again: call BEFORE editing them in place
    (csr_amd.CSR's own mutators do); the next to_handle copies afresh.  Cached copies of OTHER matrices that share one
    of csr's arrays (CSR.copy(copy_structure=False)) are dropped with it: the edit would reach them too.
    """
    mine = [a for a in (getattr(csr, 'rowptrs', None), getattr(csr, 'colinds', None), getattr(csr, 'values', None))
            if a is not None]
    with _cache_lock:
        for e in list(_cache.values()):
            if e.key[0] == id(csr) or (e.guard and any(g is a for g in e.guard for a in mine)):
                _drop_entry(e)


def _call(fn, *args):
    """
    A library call that may need device memory: on failure, give back what idle cached copies hold and retry once.
    Only for calls that leave their operands untouched when they fail (products, transposes, copies): the in-place
    operations (order_columns, unit_rows, center_rows) are never retried -- a second pass over a half-updated matrix
    would report success with wrong norms.
    """
    check(_call_rc(fn, *args))


def _call_rc(fn, *args):
    "_call without the check: the status comes back (a caller that raises its refusals its own way: combine)"
    rc = fn(*args)
    if rc == _lib.ERR_HIP:
        with _cache_lock:
            idle = any(e.refs == 0 for e in _cache.values())
        if idle:
            flush_handle_cache()
            check(lib.csrk_trim_cache())
            rc = fn(*args)
    return rc


# ---- result arrays -----------------------------------------------------------------------------------------
# The protocol returns FRESH host arrays (mult_vec: csr/kernels/numba/__init__.py:57, from_handle: :30-36).  A fresh
# np.empty of 80 MB is 20 000 unmapped pages: the device-to-host copy into it faults every one of them in (measured on
# the MI355X host: 8.3 ms against 1.43 ms into memory that has been touched before -- the product itself is 0.54 ms).
# Large results therefore come from blocks that have been through that once: a result array is a view of a LEASE on a
# block; when the caller has dropped the array and every view of it, the block goes back to the idle list (at most
# CSRK_RESULT_POOL_BYTES idle, default 2 GiB; 0 = plain np.empty everywhere).  The caller sees an ordinary writable
# ndarray that nobody else holds (`owndata` is False: its memory belongs to the lease).
_POOL_MIN = 1 << 20
_pool_lock = threading.RLock()
_pool = []                      # idle blocks: uint8 arrays whose pages are mapped
_pool_bytes = 0
_leases = {}                    # id(lease) -> weak reference: the leases behind live result arrays (an array whose base
                                # is one owns its memory alone)
# Blocks whose lease has died, not yet back on the idle list.  A lease's finalizer can run inside ANY allocation -- the
# cyclic collector frees a result array held in a reference cycle -- including allocations made while _pool_lock is held:
# it therefore takes no lock and only appends here (deque.append is atomic); _out / flush_result_pool /
# result_pool_bytes drain the queue under the lock.
_returned = collections.deque()


def _pool_cap():
    return int(os.environ.get('CSRK_RESULT_POOL_BYTES', str(2 << 30)))


def _give_back(blk, lease_id):
    _returned.append((blk, lease_id))


def _drain_returned(cap):
    "caller holds _pool_lock"
    global _pool_bytes
    while True:
        try:
            blk, lease_id = _returned.popleft()
        except IndexError:
            return
        r = _leases.get(lease_id)
        if r is not None and r() is None:      # (a NEW lease may sit at the dead one's address: its entry stays)
            del _leases[lease_id]
        if _pool_bytes + blk.nbytes <= cap:
            _pool.append(blk)
            _pool_bytes += blk.nbytes


def _is_lease(obj):
    r = _leases.get(id(obj))
    return r is not None and r() is obj


def flush_result_pool():
    "free the idle result blocks"
    global _pool_bytes
    with _pool_lock:
        _drain_returned(0)
        _pool.clear()
        _pool_bytes = 0


def result_pool_bytes():
    "bytes of idle result blocks (blocks whose arrays have been dropped included)"
    cap = _pool_cap()
    with _pool_lock:
        _drain_returned(cap)
        return _pool_bytes


def _out(shape, dtype):
    "an uninitialised array for a library call to fill: recycled memory for large results (see above)"
    global _pool_bytes
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    nbytes = n * dtype.itemsize
    cap = _pool_cap()
    if nbytes < _POOL_MIN or cap <= 0:
        return np.empty(shape, dtype=dtype)
    blk = None
    with _pool_lock:
        _drain_returned(cap)
        best = -1
        for i, b in enumerate(_pool):      # smallest idle block that fits without wasting more than a quarter
            if nbytes <= b.nbytes <= nbytes + nbytes // 4 and (best < 0 or b.nbytes < _pool[best].nbytes):
                best = i
        if best >= 0:
            blk = _pool.pop(best)
            _pool_bytes -= blk.nbytes
    if blk is None:
        blk = np.empty(nbytes, dtype=np.uint8)
    lease = (C.c_char * blk.nbytes).from_buffer(blk)
    weakref.finalize(lease, _give_back, blk, id(lease)).atexit = False
    _leases[id(lease)] = weakref.ref(lease)      # (a dict store: atomic; a finalizer running inside it only appends to _returned)
    arr = np.frombuffer(lease, dtype=dtype, count=n)      # (its base is the lease itself: what the handle cache checks)
    return arr if np.ndim(shape) == 0 or len(shape) == 1 else arr.reshape(shape)


def _create(csr, rps, cis, vs):
    out = handle_t(0)
    _call(lib.csrk_create, int(csr.nrows), int(csr.ncols), int(csr.nnz), ptr(rps), int(rps.dtype == np.dtype('i8')), ptr(cis),
          ptr(vs), _VAL_CODES[None if vs is None else vs.dtype], C.byref(out))
    return out.value


def to_handle(csr):
    """
    csr/kernels/numba/__init__.py:16-27; csr/kernels/mkl/handle.py:61-70.  Copies the
    matrix to HBM -- or hands out the idle cached copy made for this same CSR object and arrays (module docstring).
    Accepts f4/f8/absent values and int32/int64 row pointers; other value
    dtypes are widened to f8 (the reference's results are f8 whatever the storage dtype).
    """
    global _tick
    if csr.nnz > max_nnz:
        raise ValueError('CSR size {} exceeds max nnz {}'.format(csr.nnz, max_nnz))
    rps = np.ascontiguousarray(csr.rowptrs)
    if rps.dtype not in (np.dtype('i4'), np.dtype('i8')):
        rps = rps.astype(np.int64)
    cis = np.ascontiguousarray(csr.colinds, dtype=np.int32)
    vs = csr.values
    if vs is not None:
        vs = np.ascontiguousarray(vs)
        if vs.dtype not in (np.dtype('f4'), np.dtype('f8')):
            vs = vs.astype(np.float64)
    nr, nc, nnz = int(csr.nrows), int(csr.ncols), int(csr.nnz)
    mode = _cache_mode()
    guarded = mode == 'guarded'
    # small matrices are cheaper to copy than to look up; arrays that had to be converted are temporaries whose
    # addresses mean nothing on the next call; in guarded mode the class must vouch for its mutators and every array
    # must own its memory (a view's base could be written behind the guard)
    def own(a, orig):
        if a is None and orig is None:
            return True
        if not (isinstance(orig, np.ndarray) and a.ctypes.data == orig.ctypes.data):
            return False
        return not guarded or orig.base is None or _is_lease(orig.base)      # (a result array of this module: _out)
    # (a matrix with live subset_rows views is copied per handle: the views write through to its host arrays unguarded)
    cacheable = (mode != 'off' and nnz >= 4096 and (not guarded or getattr(type(csr), '__csrk_cacheable__', False))
                 and not getattr(csr, '_views', None)
                 and own(rps, csr.rowptrs) and own(cis, csr.colinds) and own(vs, csr.values))
    if cacheable:
        key = (id(csr), nr, nc, nnz, _arr_key(rps), _arr_key(cis), _arr_key(vs))
        finger = _fingerprint(rps, cis, vs)
        with _cache_lock:
            _tick += 1
            e = _cache.get(key)
            if e is not None and e.finger != finger:      # same arrays, different contents: edited in place
                _drop_entry(e)
                e = None
            if e is not None and e.refs > 0:
                # another live handle is using the cached copy (and may change it in place: order_columns,
                # unit_rows, center_rows): this one gets a copy of its own, outside the cache
                cacheable = False
                e = None
            if e is not None:
                e.refs += 1
                e.tick = _tick
                h = hip_h(e.H, nr, nc, nnz, csr)
                h._entry = e
                return h
    H = _create(csr, rps, cis, vs)
    h = hip_h(H, nr, nc, nnz, csr)
    if cacheable:
        try:
            fin = weakref.finalize(csr, _on_csr_collected, key)
        except TypeError:                                  # a CSR type without weak references (Numba structref proxy)
            return h
        fin.atexit = False
        e = _Entry()
        e.H, e.refs, e.key, e.finger, e.cached, e.fin, e.guard = H, 1, key, finger, True, fin, None
        e.bytes = rps.nbytes + cis.nbytes + (0 if vs is None else vs.nbytes)
        with _cache_lock:
            old = _cache.get(key)
            if old is not None:                            # another thread cached the same matrix meanwhile
                _drop_entry(old)
            e.tick = _tick
            _cache[key] = e
            if guarded:
                e.guard = _protect([csr.rowptrs, csr.colinds, csr.values])
        h._entry = e
    return h


def _detach(h):
    "an in-place operation is about to change this handle's device copy: it must not be handed out as `csr` again"
    e = h._entry
    if e is not None:
        with _cache_lock:
            if e.cached:
                e.cached = False
                if _cache.get(e.key) is e:
                    del _cache[e.key]
            if e.guard:
                held, e.guard = e.guard, None
                _unprotect(held)


def _info(H):
    nr, nc, nnz = C.c_int32(), C.c_int32(), C.c_int64()
    p64, vt = C.c_int(), C.c_int()
    check(lib.csrk_info(H, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(p64), C.byref(vt)))
    return nr.value, nc.value, nnz.value, p64.value, vt.value


def _wrap(H):
    nr, nc, nnz, _, _ = _info(H)
    return hip_h(H, nr, nc, nnz, None)


def from_handle(h):
    """
    csr/kernels/numba/__init__.py:30-36; csr/kernels/mkl/handle.py:95-132.  Copies the
    matrix out of HBM into a fresh host CSR; the handle may be released afterwards.
    """
    from ..csr import CSR
    nr, nc, nnz, p64, vt = _info(_live(h))
    rps = _out(nr + 1, np.int64 if p64 else np.int32)
    cis = _out(nnz, np.int32)
    vs = None if vt == _lib.VAL_NONE else _out(nnz, np.float32 if vt == _lib.VAL_F32 else np.float64)
    check(lib.csrk_export(h.H, ptr(rps), ptr(cis), ptr(vs)))
    return CSR(nr, nc, nnz, rps, cis, vs, _cast=False)


def release_handle(h):
    """
    csr/kernels/numba/__init__.py:39-44; idempotent like mkl/handle.py:144-148.  A cached device copy stays in HBM
    (idle) for the next to_handle of the same CSR; the others are freed here.
    """
    e, h._entry = h._entry, None
    H, h.H = h.H, 0
    h.csr_ref = None
    if not H:
        return
    if e is None:
        check(lib.csrk_free(H))
        return
    with _cache_lock:
        e.refs -= 1
        if e.refs == 0 and not e.cached:
            _drop_entry(e)
        elif e.cached:
            nb = C.c_int64(0)                      # the copy stays: count it with the plans it has grown meanwhile
            if lib.csrk_device_bytes(H, C.byref(nb)) == _lib.OK and nb.value > 0:
                e.bytes = nb.value
    if e.cached:
        _evict_idle(_cache_budget())


def order_columns(h):
    "csr/kernels/numba/__init__.py:47-52: sort each row by column, in place on the handle"
    _detach(h)
    check(lib.csrk_order_columns(_live(h)))         # in place: never retried (see _call)


def mult_vec(h, v):
    """
    csr/kernels/numba/__init__.py:55-67: y = A v as a fresh float64[nrows].
    v may be any real dtype of shape (ncols,).  A float32 v goes to the library as float32: Numba types the reference's
    loop by its operands, so float32 values times a float32 v is a float32 product (one rounding) added to the float64
    accumulator (csrk_spmv_f32x does the same; with float64 or absent values it widens v).  Everything else is widened to
    float64 here (exact).
    """
    v = np.asarray(v)
    if v.shape != (h.ncols,):
        raise ValueError(f'vector has shape {v.shape}, expected ({h.ncols},)')
    y = _out(h.nrows, np.float64)
    if v.dtype == np.float32:
        x = np.ascontiguousarray(v)
        _call(lib.csrk_spmv_f32x, _live(h), ptr(x), ptr(y))
        return y
    x = np.ascontiguousarray(v, dtype=np.float64)
    _call(lib.csrk_spmv, _live(h), ptr(x), ptr(y))
    return y


def mult_ab(a_h, b_h):
    "csr/kernels/numba/multiply.py:13-38: C = A B as a NEW handle the caller must release"
    assert a_h.ncols == b_h.nrows
    out = handle_t(0)
    _call(lib.csrk_spgemm_ab, _live(a_h), _live(b_h), C.byref(out))
    return _wrap(out.value)


def mult_abt(a_h, b_h):
    "csr/kernels/numba/multiply.py:41-57: C = A B^T as a NEW handle"
    assert a_h.ncols == b_h.ncols
    out = handle_t(0)
    _call(lib.csrk_spgemm_abt, _live(a_h), _live(b_h), C.byref(out))
    return _wrap(out.value)


# ---- beyond the protocol: same hot path, not kernel-dispatched in the reference ------------

def transpose(h, include_values=True):
    "csr/structure.py:240-247: transposed matrix as a NEW handle (bit-exact with the reference)"
    out = handle_t(0)
    _call(lib.csrk_transpose, _live(h), int(bool(include_values)), C.byref(out))
    return _wrap(out.value)


def from_coo(rows, cols, vals, shape):
    """
    csr/structure.py:11-67 on the device: COO arrays -> a NEW handle (entries of a row keep their
    input order, like the reference's counting sort).  `vals` may be None (structure only).
    """
    nrows, ncols = (int(v) for v in shape)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    nnz = len(rows)
    if len(cols) != nnz or (vals is not None and len(vals) != nnz):
        raise ValueError('rows, cols and vals must have the same length')
    if nnz and (rows.min() < 0 or rows.max() >= max(nrows, 1) or cols.min() < 0 or cols.max() >= max(ncols, 1)):
        raise ValueError('COO coordinates out of range')
    if vals is not None:
        vals = np.ascontiguousarray(vals)
        if vals.dtype not in (np.dtype('f4'), np.dtype('f8')):
            vals = vals.astype(np.float64)
    out = handle_t(0)
    _call(lib.csrk_from_coo, nrows, ncols, nnz, ptr(rows), ptr(cols), ptr(vals),
          _VAL_CODES[None if vals is None else vals.dtype], C.byref(out))
    return _wrap(out.value)


def row_nnzs(h):
    "csr/csr.py:432-441"
    _, _, _, p64, _ = _info(_live(h))
    out = _out(h.nrows, np.int64 if p64 else np.int32)
    check(lib.csrk_row_nnzs(h.H, ptr(out)))
    return out


def row_extent(h, row):
    "csr/_rows.py:9-13"
    s, e = C.c_int64(), C.c_int64()
    check(lib.csrk_row_extent(_live(h), int(row), C.byref(s), C.byref(e)))
    return s.value, e.value


def _row_stat(fn, h):
    _, _, _, _, vt = _info(_live(h))
    if vt == _lib.VAL_NONE:
        raise ValueError('matrix has no values')
    _detach(h)                     # unit_rows / center_rows rewrite the device copy's values
    out = _out(h.nrows, np.float32 if vt == _lib.VAL_F32 else np.float64)
    check(fn(h.H, ptr(out)))                        # in place: never retried (see _call)
    return out


def unit_rows(h):
    "csr/transform.py:29-66: unit-normalise rows IN PLACE on the handle; returns the norms"
    return _row_stat(lib.csrk_unit_rows, h)


def center_rows(h):
    "csr/transform.py:13-26: mean-centre rows IN PLACE on the handle; returns the means"
    return _row_stat(lib.csrk_center_rows, h)


def pick_rows(h, rows, include_values=True):
    "csr/csr.py:347-364 on the device: NEW handle with the given rows (in order, repeats allowed)"
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = handle_t(0)
    _call(lib.csrk_pick_rows, _live(h), rows.ctypes.data_as(C.c_void_p), rows.size, int(bool(include_values)), C.byref(out))
    return _wrap(out.value)


def filter_zeros(h):
    "csr/_struct.py:61-76 on the device: NEW handle without exact-zero entries"
    out = handle_t(0)
    _call(lib.csrk_filter_zeros, _live(h), C.byref(out))
    return _wrap(out.value)


_TOPK_ORDERS = {'descending': _lib.TOPK_BY_VALUE, 'storage': _lib.TOPK_STORAGE}


def _is_int(v):
    "an integer (a bool is none)"
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _is_real(v):
    "a real number (a bool is none)"
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _limits(fn, n):
    "the n compile-time constants a csrk_*_limits entry reports, as a tuple"
    out = (C.c_int64 * n)()
    check(fn(out, n))
    return tuple(out)


def topk_args(k, min_value, order):
    "(k, min_value, order code) as the library takes them; ValueError for anything it would refuse"
    if not _is_int(k):
        raise ValueError(f'k must be an integer, not {k!r}')
    if k < 1:
        raise ValueError(f'k must be at least 1, not {k}')
    mv = -np.inf if min_value is None else float(min_value)
    if mv != mv:
        raise ValueError('min_value is NaN')
    if order not in _TOPK_ORDERS:
        raise ValueError(f"order must be 'descending' or 'storage', not {order!r}")
    return min(int(k), int(max_nnz)), mv, _TOPK_ORDERS[order]


def topk_rows(h, k, min_value=None, order='descending'):
    """
    Row top-k on the device: NEW handle whose rows hold each row's k largest entries that are not below min_value (None:
    no threshold), best first (order='descending') or in the order they had in the row (order='storage').  NaN ranks
    above +Inf, -0.0 ties with +0.0, ties go to the entry stored earlier; indices and values are copied bit for bit
    (include/csrk.h).  Not a reference entry point.
    """
    k, mv, code = topk_args(k, min_value, order)
    out = handle_t(0)
    _call(lib.csrk_topk_rows, _live(h), k, mv, code, C.byref(out))
    return _wrap(out.value)


def topk_limits():
    "(longest row ranked by one wavefront, winners a large-class workgroup orders in LDS, its threads, longest medium row)"
    return _limits(lib.csrk_topk_limits, 4)


_COMBINE_OPS = {'add': _lib.COMBINE_ADD, 'multiply': _lib.COMBINE_MUL, 'keep': _lib.COMBINE_KEEP, 'drop': _lib.COMBINE_DROP}


def combine_args(a, b, op, alpha=1.0, beta=1.0):
    """
    (op code, alpha, beta) as the library takes them; ValueError for an unknown op, a non-real alpha or beta, or operands
    (handles or CSRs: anything with nrows and ncols) of different shapes
    """
    if not isinstance(op, str) or op not in _COMBINE_OPS:
        raise ValueError(f"op must be 'add', 'multiply', 'keep' or 'drop', not {op!r}")
    for name, v in (('alpha', alpha), ('beta', beta)):
        if not _is_real(v):
            raise ValueError(f'{name} must be a real number, not {v!r}')
    if (a.nrows, a.ncols) != (b.nrows, b.ncols):
        raise ValueError(f'operands of different shapes: {a.nrows} x {a.ncols} and {b.nrows} x {b.ncols}')
    return _COMBINE_OPS[op], float(alpha), float(beta)


def combine(a_h, b_h, op, alpha=1.0, beta=1.0):
    """
    Two matrices entry by entry on the device: NEW handle of A's shape (include/csrk.h, csrk_combine).
      'add'       alpha A + beta B over the union of the patterns    (float64; each product and the sum rounded on its own)
      'multiply'  a b over the intersection                          (float64)
      'keep'      the entries of A whose position B stores           (A's storage order, indices and values bit for bit)
      'drop'      the entries of A whose position B does not store   (the same)
    'add' and 'multiply' need both operands canonical (every row strictly ascending in column), 'keep' and 'drop' only
    B: A may be unsorted and repeat columns.  The library refuses a non-canonical operand with CsrkError (its message
    names the operand and a row); order_columns sorts, coalesce sorts and merges.  a_h may be b_h.  Not a reference entry point.
    """
    code, al, be = combine_args(a_h, b_h, op, alpha, beta)
    out = handle_t(0)
    rc = _call_rc(lib.csrk_combine, _live(a_h), _live(b_h), code, al, be, C.byref(out))
    if rc != _lib.OK:
        raise _lib.CsrkError(rc, _lib.last_error())
    return _wrap(out.value)


def combine_limits():
    "(entries a wavefront takes per step, entries a workgroup takes per step, largest len_a + len_b of the wavefront class)"
    return _limits(lib.csrk_combine_limits, 3)


_DUPLICATES = {'sum': _lib.DUP_SUM, 'first': _lib.DUP_FIRST, 'last': _lib.DUP_LAST, 'max': _lib.DUP_MAX, 'min': _lib.DUP_MIN}


def coalesce_args(duplicates):
    "the dup code as the library takes it; ValueError for anything but 'sum', 'first', 'last', 'max', 'min'"
    if not isinstance(duplicates, str) or duplicates not in _DUPLICATES:
        raise ValueError(f"duplicates must be 'sum', 'first', 'last', 'max' or 'min', not {duplicates!r}")
    return _DUPLICATES[duplicates]


def coalesce(h, duplicates='sum'):
    """
    The canonical form of the handle's matrix on the device: NEW handle of the same shape, every row strictly ascending in
    column, one entry per distinct (row, column) (include/csrk.h, csrk_coalesce).  The entries of a row that share a column
    become, in their storage order:
      'sum'    ((v0 + v1) + v2) + ...   each add rounded in the values' dtype; an exact zero stays stored
      'first'  v0                       'last'  the one stored last              (bit for bit)
      'max'    the earliest stored of the largest      'min'  the latest stored of the smallest      (bit for bit; NaN
               ranks above +Inf, -0.0 ties with +0.0: topk_rows' order)
    Values keep their dtype; a structure-only matrix stays structure-only.  h is not modified.  The result may go straight
    into combine.  Not a reference entry point.
    """
    code = coalesce_args(duplicates)
    out = handle_t(0)
    _call(lib.csrk_coalesce, _live(h), code, C.byref(out))
    return _wrap(out.value)


def coalesce_last_route():
    "what this thread's last coalesce did: 0 copied a canonical matrix, 1 merged without sorting, 2 sorted and merged"
    r = C.c_int(0)
    check(lib.csrk_coalesce_last_route(C.byref(r)))
    return r.value


def is_canonical(h):
    """
    (True, None) when every row of the handle's matrix is strictly ascending in column, else (False, the first row that
    is not).  Looked at on the device once per handle; combine and coalesce use the same answer.
    """
    ok, row = C.c_int(0), C.c_int32(-1)
    _call(lib.csrk_is_canonical, _live(h), C.byref(ok), C.byref(row))
    return (True, None) if ok.value else (False, row.value)


def values_of(h):
    "copy only the value array out of HBM (after an in-place row operation)"
    _, _, nnz, _, vt = _info(_live(h))
    if vt == _lib.VAL_NONE:
        return None
    vs = _out(nnz, np.float32 if vt == _lib.VAL_F32 else np.float64)
    check(lib.csrk_export(h.H, None, None, ptr(vs)))
    return vs


def mult_dense(h, B):
    """
    C = A B for a dense row-major B [ncols x k] (BASELINE.json configs[2]); equals
    mult_ab(A, CSR(B)) densified.  Not a reference entry point.
    """
    B = np.ascontiguousarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != h.ncols:
        raise ValueError(f'panel has shape {B.shape}, expected ({h.ncols}, k)')
    k = B.shape[1]
    out = _out((h.nrows, k), np.float64)
    _call(lib.csrk_spmm_dense, _live(h), ptr(B), k, k, ptr(out), k)
    return out


_PANEL_CODES = {np.dtype('f4'): _lib.VAL_F32, np.dtype('f8'): _lib.VAL_F64}


def _panel_pair(U, V, dtype_error=None):
    """
    what two panels must agree on: both 2-D, one dtype, one k >= 1.  dtype_error: the caller's words for a shared dtype that
    is no panel dtype, raised where that caller has always raised them (once the dtypes are known to agree, before the
    columns are compared); None leaves the dtype to _panel.
    """
    if U.ndim != 2 or V.ndim != 2:
        raise ValueError(f'panels must be 2-D, not of shapes {U.shape} and {V.shape}')
    if U.dtype != V.dtype:
        raise ValueError(f'U and V must have the same dtype, not {U.dtype} and {V.dtype}')
    if dtype_error and U.dtype not in _PANEL_CODES:
        raise ValueError(f'{dtype_error}, not {U.dtype}')
    if U.shape[1] != V.shape[1]:
        raise ValueError(f'U and V have {U.shape[1]} and {V.shape[1]} columns')
    if U.shape[1] == 0:
        raise ValueError('panels have no columns (k = 0)')


def _row_range(rows, nrows):
    "(begin, end) from rows = None (all of the nrows rows) or a pair of integers that is a range within them"
    if rows is None:
        return 0, int(nrows)
    try:
        rb, re_ = rows
    except (TypeError, ValueError):
        raise ValueError(f'rows must be (begin, end), not {rows!r}') from None
    if not (_is_int(rb) and _is_int(re_)):
        raise ValueError(f'rows must be two integers, not {rows!r}')
    rb, re_ = int(rb), int(re_)
    if not 0 <= rb <= re_ <= nrows:
        raise ValueError(f'rows ({rb}, {re_}) is not a range within the {nrows} rows')
    return rb, re_


def _panel(P, rows, name):
    "a 2-D float32 / float64 panel of `rows` rows as (array, ld): a row-major view with unit column stride keeps its row stride"
    if P.ndim != 2:
        raise ValueError(f'{name} must be 2-D, not of shape {P.shape}')
    if P.dtype not in _PANEL_CODES:
        raise ValueError(f'{name} must be float32 or float64, not {P.dtype}')
    if P.shape[0] != rows:
        raise ValueError(f'{name} has {P.shape[0]} rows, expected {rows}')
    es = P.dtype.itemsize
    if P.strides[1] == es and P.strides[0] % es == 0 and P.strides[0] >= P.shape[1] * es:
        return P, P.strides[0] // es
    P = np.ascontiguousarray(P)
    return P, P.shape[1]


def sddmm(h, U, V, scale=False):
    """
    Sampled dense-dense product: for every stored entry (i, j) of the handle's matrix, in its storage order,
    dot(U[i, :], V[j, :]) -- times the entry's value with scale=True (1.0 for a structure-only matrix) -- as a fresh
    float64[nnz].  U [nrows x k] and V [ncols x k] are both float32 or both float64; the sums are float64 in a fixed order
    (include/csrk.h).  Not a reference entry point.
    """
    U, V = np.asarray(U), np.asarray(V)
    _panel_pair(U, V)      # (their dtype is left to _panel: "U must be float32 or float64")
    U, ldu = _panel(U, h.nrows, 'U')
    V, ldv = _panel(V, h.ncols, 'V')
    k = U.shape[1]
    out = _out(h.nnz, np.float64)
    _call(lib.csrk_sddmm, _live(h), ptr(U), ldu, ptr(V), ldv, k, _PANEL_CODES[U.dtype], int(bool(scale)), ptr(out))
    return out


def gram_limits():
    "(largest k, entries staged per step, largest k of the 16-lane class, of the wavefront class, of the one-tile workgroup class)"
    return _limits(lib.csrk_gram_limits, 5)


def gram_args(h, V, rows=None, base=None):
    """
    (V, ldv, k, panel code, row_begin, row_end, base) as the library takes them; ValueError for anything it would refuse
    as invalid.  h is anything with nrows and ncols (a handle or a CSR); no library call is made.
    """
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError(f'V must be 2-D, not of shape {V.shape}')
    if V.dtype not in _PANEL_CODES:
        raise ValueError(f'V must be float32 or float64, not {V.dtype}')
    if V.shape[1] == 0:
        raise ValueError('V has no columns (k = 0)')
    V, ldv = _panel(V, h.ncols, 'V')
    k = V.shape[1]
    rb, re_ = _row_range(rows, h.nrows)
    if base is not None:
        base = np.asarray(base)
        if base.dtype != np.float64 or base.shape != (k, k):
            raise ValueError(f'base must be float64 of shape ({k}, {k}), not {base.dtype} of shape {base.shape}')
        base = np.ascontiguousarray(base)
    return V, ldv, k, _PANEL_CODES[V.dtype], rb, re_, base


def gram_rows(h, V, scale=False, rows=None, base=None):
    """
    One k x k Gram matrix per row: for each row i of rows = (begin, end) (None: all rows), base + the sum over the row's
    stored entries (i, j), in storage order, of w V[j, :]^T V[j, :], w = 1 or, with scale=True, the entry's value (1.0 for a
    structure-only matrix) -- as a fresh float64 [end - begin, k, k], exactly symmetric.  V [ncols x k] is float32 or
    float64; base is None or float64 [k, k] of which the lower triangle is read.  Each element is one serial chain of a
    rounded multiply and a fused multiply-add per entry (include/csrk.h, csrk_gram_rows).  Not a reference entry point.
    """
    V, ldv, k, code, rb, re_, base = gram_args(h, V, rows, base)
    out = _out((re_ - rb, k, k), np.float64)
    _call(lib.csrk_gram_rows, _live(h), rb, re_, ptr(V), ldv, k, code, int(bool(scale)), ptr(base), ptr(out))
    return out


def als_limits():
    "(largest k, entries staged per step, largest k of the 16-lane class, of the wavefront class, of the one-tile workgroup class)"
    return _limits(lib.csrk_als_limits, 5)


_RHS_CODES = {'ones': _lib.ALS_RHS_ONES, 'values': _lib.ALS_RHS_VALUES, 'one_plus_values': _lib.ALS_RHS_ONE_PLUS}


def solve_args(G, b):
    "(G, b, n, k) as the library takes them; ValueError for anything it would refuse as invalid.  No library call is made."
    G, b = np.asarray(G), np.asarray(b)
    if G.ndim != 3 or G.shape[1] != G.shape[2] or G.dtype != np.float64:
        raise ValueError(f'G must be float64 of shape (n, k, k), not {G.dtype} of shape {G.shape}')
    n, k = G.shape[0], G.shape[1]
    if k == 0:
        raise ValueError('the systems have no unknowns (k = 0)')
    if b.dtype != np.float64 or b.shape != (n, k):
        raise ValueError(f'b must be float64 of shape ({n}, {k}), not {b.dtype} of shape {b.shape}')
    return np.ascontiguousarray(G), np.ascontiguousarray(b), n, k


def solve_blocks(G, b):
    """
    Solve n symmetric k x k systems G[s] x[s] = b[s]: (x float64 [n, k], info int32 [n]).  Only the lower triangle of each
    G[s] is read.  An LDL^T factorisation without pivoting in a fixed order of fused multiply-adds (include/csrk.h, rule
    S): the same bits whatever the launch.  info[s] is 0, or j + 1 for the first pivot j that is not positive (x[s] is then
    Inf / NaN or meaningless).  Not a reference entry point.
    """
    G, b, n, k = solve_args(G, b)
    x, info = _out((n, k), np.float64), np.zeros(n, np.int32)
    check(lib.csrk_solve_blocks(n, k, ptr(G), ptr(b), k, ptr(x), k, ptr(info)))
    return x, info


def als_args(h, V, rhs='values', base=None, lam_n=0.0, rows=None):
    "gram_args' tuple + (rhs code, lam_n); ValueError for anything the library would refuse as invalid.  No library call."
    args = gram_args(h, V, rows, base)
    if not isinstance(rhs, str) or rhs not in _RHS_CODES:
        raise ValueError(f'rhs must be one of {sorted(_RHS_CODES)}, not {rhs!r}')
    if not _is_real(lam_n):
        raise ValueError(f'the per-entry ridge must be one real number, not {lam_n!r}')
    return args + (_RHS_CODES[rhs], float(lam_n))


def als_rows(h, V, scale=False, rhs='values', base=None, lam_n=0.0, rows=None):
    """
    One ALS half-step: for each row i of rows = (begin, end) (None: all rows) solve
        (base + sum_e w_e v_j v_j^T + lam_n n_i I) u_i = sum_e c_e v_j
    over the row's n_i stored entries e = (i, j) in storage order, v_j = V[j, :]: (U float64 [end - begin, k], info int32).
    w is 1 or (scale=True) the entry's value; c is 1 (rhs='ones'), the value ('values') or 1 + the value
    ('one_plus_values'); a structure-only matrix counts every value as 1.0.  The block is csrk_gram_rows', built and
    factorised in registers and never written; the solve is solve_blocks' (include/csrk.h, rules A and S).  info[i] is 0, or
    j + 1 for the first pivot j of row i that is not positive.  Not a reference entry point.
    """
    V, ldv, k, code, rb, re_, base, rcode, lam_n = als_args(h, V, rhs, base, lam_n, rows)
    out, info = _out((re_ - rb, k), np.float64), np.zeros(re_ - rb, np.int32)
    _call(lib.csrk_als_rows, _live(h), rb, re_, ptr(V), ldv, k, code, int(bool(scale)), rcode, ptr(base), lam_n, ptr(out), k,
          ptr(info))
    return out, info


def als_cg_limits():
    "(largest k, lanes of a row's team, entries a team has in flight per step of its entry loop)"
    return _limits(lib.csrk_als_cg_limits, 3)


def als_cg_long_limits():
    """
    the long-row class of als_rows_cg (include/csrk.h, rule C11): (default L, threads of a long row's workgroup, S = rows
    whose lengths one workgroup scans, C for float64 k <= 64, float64 k <= 128, float32 k <= 64, float32 k <= 128 = entries
    of one chunk of the row's LDS image, image buffers)
    """
    return _limits(lib.csrk_als_cg_long_limits, 8)


def als_cg_set_long(entries):
    """
    From how many entries a row of als_rows_cg takes a whole workgroup: an integer >= 1; 0 turns the class off; None (or
    -1) follows the environment variable CSRK_ALS_CG_LONG (a decimal count; unset: the default).  Process-wide.  No result
    bit depends on it.
    """
    if entries is None:
        entries = -1
    if not _is_int(entries) or entries < -1 or entries > 2 ** 63 - 1:
        raise ValueError(f'entries must be None, -1, 0 or a count of at least 1, not {entries!r}')
    check(lib.csrk_als_cg_set_long(int(entries)))


def als_cg_get_long():
    "the L in force: a row of at least that many entries is a long row of als_rows_cg; 0: the class is off"
    v = C.c_int64(0)
    check(lib.csrk_als_cg_get_long(C.byref(v)))
    return v.value


def als_cg_last_stats():
    """
    what this thread's last als_rows_cg did (include/csrk.h, csrk_als_cg_last_stats): (1 if it launched, the L in force,
    1 if the long rows' launch was issued, its workgroups, the rows it solved, their entries); all 0 after a refused call
    """
    return _limits(lib.csrk_als_cg_last_stats, 6)


def als_cg_args(h, V, rhs='values', base=None, lam=0.0, lam_n=0.0, rows=None, steps=3, x0=None, tol=0.0):
    """
    als_args' tuple (with the constant ridge lam before lam_n) + (steps, tol2, x0); ValueError for anything the library
    would refuse as invalid.  tol is a residual 2-norm: the library takes its square.  No library call.
    """
    if not _is_real(lam):
        raise ValueError(f'the ridge must be one real number, not {lam!r}')
    V, ldv, k, code, rb, re_, base, rcode, lam_n = als_args(h, V, rhs, base, lam_n, rows)
    if not _is_int(steps) or steps < 0 or steps > 2 ** 31 - 1:
        raise ValueError(f'steps must be an integer that is not negative, not {steps!r}')
    if not _is_real(tol) or not float(tol) >= 0.0:
        raise ValueError(f'tol must be a real number that is not negative, not {tol!r}')
    if x0 is not None:
        x0 = np.asarray(x0)
        if x0.dtype != np.float64 or x0.shape != (re_ - rb, k):
            raise ValueError(f'x0 must be float64 of shape ({re_ - rb}, {k}), not {x0.dtype} of shape {x0.shape}')
        x0 = np.ascontiguousarray(x0)
    tol = float(tol)
    return V, ldv, k, code, rb, re_, base, rcode, float(lam), lam_n, int(steps), tol * tol, x0


def als_rows_cg(h, V, scale=False, rhs='values', base=None, lam=0.0, lam_n=0.0, rows=None, steps=3, x0=None, tol=0.0):
    """
    One ALS half-step by conjugate gradient: for each row i of rows = (begin, end) (None: all rows) at most `steps` CG steps
    from x0's row (None: from zero) on als_rows' system with the ridge lam + lam_n n_i on the diagonal,
        (base + sum_e w_e v_j v_j^T + (lam + lam_n n_i) I) u_i = sum_e c_e v_j
    without forming the k x k block: (U float64 [end - begin, k], resid float64, taken int32).  A row stops early once the
    squared residual of the recurrence is no longer above tol^2; resid is that squared residual at the stop and taken the
    steps made.  base is read as stored, all of it (als_rows reads the lower triangle): pass a symmetric matrix.  Every
    output is a fixed chain of fused multiply-adds (include/csrk.h, rule C).  Not a reference entry point.
    """
    V, ldv, k, code, rb, re_, base, rcode, lam, lam_n, steps, tol2, x0 = als_cg_args(h, V, rhs, base, lam, lam_n, rows, steps, x0, tol)
    n = re_ - rb
    out, resid, taken = _out((n, k), np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    _call(lib.csrk_als_rows_cg, _live(h), rb, re_, ptr(V), ldv, k, code, int(bool(scale)), rcode, ptr(base), lam, lam_n, steps, tol2,
          ptr(x0), k, ptr(out), k, ptr(resid), ptr(taken))
    return out, resid, taken


def panel_gram_limits():
    "(largest k, R = the rows of one chunk of panel_gram's sum)"
    return _limits(lib.csrk_panel_gram_limits, 2)


def panel_gram_args(V, ridge=0.0):
    "(V, ldv, n, k, panel code, ridge) as the library takes them; ValueError for anything it would refuse as invalid.  No library call."
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError(f'V must be 2-D, not of shape {V.shape}')
    if V.dtype not in _PANEL_CODES:
        raise ValueError(f'V must be float32 or float64, not {V.dtype}')
    if V.shape[1] == 0:
        raise ValueError('V has no columns (k = 0)')
    if not _is_real(ridge) or float(ridge) != float(ridge):
        raise ValueError(f'ridge must be one real number that is not NaN, not {ridge!r}')
    V, ldv = _panel(V, V.shape[0], 'V')
    return V, ldv, V.shape[0], V.shape[1], _PANEL_CODES[V.dtype], float(ridge)


def panel_gram(V, ridge=0.0):
    """
    G = V^T V + ridge I as a fresh float64 [k, k], exactly symmetric: the `base` of implicit-feedback ALS (als_rows,
    als_rows_cg).  V [n x k] is float32 or float64.  Each element is a chain of fused multiply-adds over every chunk of R
    rows (panel_gram_limits) and a fixed tree of rounded additions over the chunks; the ridge is added to the diagonal last
    (include/csrk.h, rule P).  No rows give ridge I.  Not a reference entry point.
    """
    V, ldv, n, k, code, ridge = panel_gram_args(V, ridge)
    out = _out((k, k), np.float64)
    _call(lib.csrk_panel_gram, n, k, ptr(V), ldv, code, ridge, ptr(out))
    return out


def als_objective_limits():
    "(largest k, L = the elements of one serial chunk of the objective's sums, lanes of a row's team, entries in flight per step)"
    return _limits(lib.csrk_als_objective_limits, 4)


def _factor_pair(a, U, V):
    "(U, ldu, V, ldv, k) for float64 factor panels of a's rows and columns; ValueError otherwise.  No library call."
    U, V = np.asarray(U), np.asarray(V)
    _panel_pair(U, V)
    if U.dtype != np.float64:
        raise ValueError(f'U and V must be float64, not {U.dtype}')
    U, ldu = _panel(U, a.nrows, 'U')
    V, ldv = _panel(V, a.ncols, 'V')
    return U, ldu, V, ldv, U.shape[1]


def als_objective_args(a, at, U, V, rhs='values', lam=0.0, lam_n=0.0, rows=None):
    """
    (U, ldu, V, ldv, k, rhs code, lam, lam_n, row_begin, row_end) as the library takes them; ValueError for anything it would
    refuse as invalid.  a and at are anything with nrows, ncols and nnz (handles or CSRs); at may be None (the rows form).
    No library call is made.
    """
    U, ldu, V, ldv, k = _factor_pair(a, U, V)
    if at is not None and (at.nrows, at.ncols, at.nnz) != (a.ncols, a.nrows, a.nnz):
        raise ValueError(f'the second matrix is {at.nrows} x {at.ncols} with {at.nnz} entries: not the shape of the transpose of '
                         f'{a.nrows} x {a.ncols} with {a.nnz}')
    if not isinstance(rhs, str) or rhs not in _RHS_CODES:
        raise ValueError(f'rhs must be one of {sorted(_RHS_CODES)}, not {rhs!r}')
    if not _is_real(lam) or not _is_real(lam_n):
        raise ValueError(f'the ridges must be real numbers, not {lam!r} and {lam_n!r}')
    rb, re_ = _row_range(rows, a.nrows)
    return U, ldu, V, ldv, k, _RHS_CODES[rhs], float(lam), float(lam_n), rb, re_


def als_objective_rows(h, U, V, scale=False, rhs='values', lam=0.0, lam_n=0.0, data=True, rows=None):
    """
    The ALS objective row by row, float64 [end - begin]: for each row i of rows = (begin, end) (None: all rows)
        J_i = sum_e (g_e - 2 c_e) s_e + (lam + lam_n n_i) |u_i|^2,   s_e = u_i . v_j,  g_e = w_e s_e (scale) or s_e,
    with w and c as in als_rows; data=False leaves the entries out (V is not read): the regulariser alone.  U [nrows x k]
    and V [ncols x k] are float64.  One fused multiply-add per entry in storage order (include/csrk.h, rule J1).  Not a
    reference entry point.
    """
    U, ldu, V, ldv, k, rcode, lam, lam_n, rb, re_ = als_objective_args(h, None, U, V, rhs, lam, lam_n, rows)
    out = _out(re_ - rb, np.float64)
    _call(lib.csrk_als_objective_rows, _live(h), rb, re_, ptr(U), ldu, ptr(V), ldv, k, int(bool(scale)), rcode, int(bool(data)), lam,
          lam_n, ptr(out))
    return out


def als_objective(a_h, at_h, U, V, scale=False, rhs='values', implicit=False, lam=0.0, lam_n=0.0):
    """
    The ALS objective, one float: the sum of als_objective_rows over a_h's rows, of the regulariser over at_h's rows (the
    transpose: only its row lengths are read) and, with implicit=True, of <U^T U, V^T V>, the all-pairs term of implicit
    ALS -- every sum in a fixed order (include/csrk.h, rules J2 and T).  It is the usual loss MINUS a constant that does not
    depend on the factors: sum a_e^2 for explicit ALS (scale=False, rhs='values'), sum (1 + a_e) for Hu-Koren implicit ALS
    (scale=True, rhs='one_plus_values', implicit=True).  Not a reference entry point.
    """
    U, ldu, V, ldv, k, rcode, lam, lam_n, _, _ = als_objective_args(a_h, at_h, U, V, rhs, lam, lam_n)
    out = np.zeros(1, np.float64)
    _call(lib.csrk_als_objective, _live(a_h), _live(at_h), ptr(U), ldu, ptr(V), ldv, k, int(bool(scale)), rcode, int(bool(implicit)),
          lam, lam_n, ptr(out))
    return float(out[0])


_SOLVER_CODES = {'exact': 0, 'cg': 1}


def als_fit_args(a, at, U0, V0, sweeps=10, solver='cg', steps=3, rhs='values', lam=0.0, lam_n=0.0, tol=0.0):
    """
    (U, V, k, sweeps, solver code, steps, tol2, rhs code, lam, lam_n) as the library takes them -- U and V fresh packed
    float64 copies of the start factors, which the fit overwrites; ValueError for anything it would refuse as invalid.
    tol is a residual 2-norm: the library takes its square.  No library call is made.
    """
    U, _, V, _, k, rcode, lam, lam_n, _, _ = als_objective_args(a, at, U0, V0, rhs, lam, lam_n)
    if not _is_int(sweeps) or sweeps < 0 or sweeps > 2 ** 30:
        raise ValueError(f'sweeps must be an integer that is not negative, not {sweeps!r}')
    if not isinstance(solver, str) or solver not in _SOLVER_CODES:
        raise ValueError(f'solver must be one of {sorted(_SOLVER_CODES)}, not {solver!r}')
    if not _is_int(steps) or steps < 0 or steps > 2 ** 31 - 1:
        raise ValueError(f'steps must be an integer that is not negative, not {steps!r}')
    if not _is_real(tol) or not float(tol) >= 0.0:
        raise ValueError(f'tol must be a real number that is not negative, not {tol!r}')
    tol = float(tol)
    return np.array(U, dtype=np.float64, order='C'), np.array(V, dtype=np.float64, order='C'), k, int(sweeps), _SOLVER_CODES[solver], \
        int(steps), tol * tol, rcode, lam, lam_n


def als_fit(a_h, at_h, U0, V0, sweeps=10, solver='cg', steps=3, scale=False, rhs='values', implicit=False, lam=0.0, lam_n=0.0, tol=0.0,
            objective=False):
    """
    `sweeps` sweeps of alternating least squares with both factor panels on the device throughout: (U, V, objective, bad).
    a_h is the matrix, at_h its transpose with values; U0 [nrows x k] and V0 [ncols x k] are the float64 start factors (the
    library draws no random numbers).  A sweep is a half-step for U and one for V -- solver 'cg': als_rows_cg, `steps` steps
    from the current factors; 'exact': als_rows -- with base = V^T V (panel_gram) under implicit=True and lam, lam_n as the
    ridges; the result equals the caller's own loop over panel_gram, als_rows[_cg] and als_objective bit for bit
    (include/csrk.h, rule F).  objective=True: a float64 [sweeps + 1] array, als_objective before the first sweep and after
    each; else None.  bad: int64 [2 sweeps], per half-step the rows whose system had a pivot that is not positive
    (always 0 for 'cg').  Not a reference entry point.
    """
    U, V, k, sweeps, scode, steps, tol2, rcode, lam, lam_n = als_fit_args(a_h, at_h, U0, V0, sweeps, solver, steps, rhs, lam, lam_n, tol)
    obj = np.zeros(sweeps + 1, np.float64) if objective else None
    bad = np.zeros(2 * sweeps, np.int64)
    _call(lib.csrk_als_fit, _live(a_h), _live(at_h), k, sweeps, scode, steps, tol2, int(bool(scale)), rcode, int(bool(implicit)), lam,
          lam_n, ptr(U), k, ptr(V), k, ptr(obj), ptr(bad))
    return U, V, obj, bad


def topk_scores_limits():
    "(largest k, largest n, rows per workgroup, items per tile, factors per LDS chunk, list entries per row for n <= 32)"
    return _limits(lib.csrk_topk_scores_limits, 6)


def topk_scores_args(h, U, V, n, min_score=None, rows=None):
    """
    (U, ldu, V, ldv, n_items, k, panel code, n, min_score, row_begin, row_end) as the library takes them; ValueError for
    anything it would refuse as invalid.  h is anything with nrows and ncols (a handle or a CSR: the seen pairs) or None
    (nothing seen: U's rows and V's rows give the shape); no library call is made.
    """
    U, V = np.asarray(U), np.asarray(V)
    _panel_pair(U, V, 'U and V must be float32 or float64')
    nrows = U.shape[0] if h is None else int(h.nrows)
    n_items = V.shape[0] if h is None else int(h.ncols)
    if nrows > np.iinfo('i4').max or n_items > np.iinfo('i4').max:
        raise ValueError(f'{nrows} rows or {n_items} items are more than 32-bit indices hold')
    U, ldu = _panel(U, nrows, 'U')
    V, ldv = _panel(V, n_items, 'V')
    if not _is_int(n):
        raise ValueError(f'n must be an integer, not {n!r}')
    if n < 1:
        raise ValueError(f'n must be at least 1, not {n}')
    if not (min_score is None or _is_real(min_score)):
        raise ValueError(f'min_score must be one real number or None, not {min_score!r}')
    ms = -np.inf if min_score is None else float(min_score)
    if ms != ms:
        raise ValueError('min_score is NaN')
    rb, re_ = _row_range(rows, nrows)
    return U, ldu, V, ldv, n_items, U.shape[1], _PANEL_CODES[U.dtype], min(int(n), np.iinfo('i4').max), ms, rb, re_


def topk_scores(h, U, V, n, min_score=None, rows=None):
    """
    Recommendations from factors: for each row i of rows = (begin, end) (None: all rows) the n best items j by the score
    dot(U[i, :], V[j, :]) among those the handle's matrix does not store in row i (h = None: nothing is left out) and whose
    score is not below min_score (None: no threshold) -- (items int32 [m, n], scores float64 [m, n], counts int32 [m]),
    best first, padded with item -1 and score -inf beyond counts[i].  U [nrows x k] and V [ncols x k] are both float32 or
    both float64; a score is one chain of k fused multiply-adds in float64; NaN ranks above +Inf, -0.0 ties with +0.0, ties
    go to the smaller item (include/csrk.h, csrk_topk_scores).  The handle's matrix must be canonical.  Not a reference
    entry point.
    """
    U, ldu, V, ldv, n_items, k, code, n, ms, rb, re_ = topk_scores_args(h, U, V, n, min_score, rows)
    m = re_ - rb
    lim = topk_scores_limits()
    if k > lim[0] or n > lim[1]:      # the library's refusal, before any result array is made
        check(lib.csrk_topk_scores(0 if h is None else _live(h), rb, re_, ptr(U), ldu, ptr(V), ldv, n_items, k, code, n, ms, None, n,
                                   None, n, None))
        raise ValueError(f'k = {k} or n = {n} is above the limits {lim[:2]}')
    items, scores, counts = np.empty((m, n), np.int32), np.empty((m, n), np.float64), np.zeros(m, np.int32)
    _call(lib.csrk_topk_scores, 0 if h is None else _live(h), rb, re_, ptr(U), ldu, ptr(V), ldv, n_items, k, code, n, ms, ptr(items),
          n, ptr(scores), n, ptr(counts))
    return items, scores, counts


def topk_scores_for_limits():
    "(most splits, workgroups that fill the card for n <= 32, above that, workspace bytes per (row, split) at n = 1, per further unit of n)"
    return _limits(lib.csrk_topk_scores_for_limits, 5)


def _splits(splits):
    "the library's splits argument (0: automatic) from None or an integer >= 1"
    if splits is None:
        return 0
    if not _is_int(splits) or splits < 1:
        raise ValueError(f'splits must be None or an integer that is at least 1, not {splits!r}')
    return min(int(splits), np.iinfo('i4').max)


def _row_list(users, nrows):
    "users as a contiguous int32 list of row indices in [0, nrows): 1-D, integers, any order, repeats allowed; else ValueError"
    users = np.asarray(users, np.int32) if isinstance(users, (list, tuple)) and len(users) == 0 else np.asarray(users)
    if users.ndim != 1:
        raise ValueError(f'users must be 1-D, not of shape {users.shape}')
    if users.dtype == np.bool_ or not np.issubdtype(users.dtype, np.integer):
        raise ValueError(f'users must hold integers, not {users.dtype}')
    bad = np.flatnonzero((users < 0) | (users >= nrows))
    if len(bad):
        raise ValueError(f'users[{int(bad[0])}] = {int(users[bad[0]])} is outside [0, {nrows})')
    return np.ascontiguousarray(users, dtype=np.int32)


def topk_scores_for_workspace(n_rows, n_items, n, splits=None):
    """
    (splits_used, bytes): into how many ranges topk_scores_for cuts the items for n_rows listed rows, n_items items and
    lists of n (splits=None: as many as fill the card), and the bytes of the workspace the device form needs for it (0 for
    one range).  From the library's constants alone: no device is touched.
    """
    for name, v in (('n_rows', n_rows), ('n_items', n_items), ('n', n)):
        if not _is_int(v):
            raise ValueError(f'{name} must be an integer, not {v!r}')
    if n_items > np.iinfo('i4').max:
        raise ValueError(f'{n_items} items are more than 32-bit indices hold')
    used, nbytes = C.c_int32(0), C.c_int64(0)
    check(lib.csrk_topk_scores_for_workspace(int(n_rows), int(n_items), min(int(n), np.iinfo('i4').max), _splits(splits), C.byref(used),
                                             C.byref(nbytes)))
    return used.value, nbytes.value


def topk_scores_for_args(h, users, U, V, n, min_score=None, splits=None):
    """
    (users int32, U, ldu, V, ldv, n_items, k, panel code, n, min_score, splits, u_rows) as the library takes them; ValueError
    for anything it would refuse as invalid.  h is as in topk_scores_args; users is a 1-D array of integer row indices in any
    order, repeats allowed; no library call is made.
    """
    U, ldu, V, ldv, n_items, k, code, n, ms, _, nrows = topk_scores_args(h, U, V, n, min_score, None)
    users = _row_list(users, nrows)
    return users, U, ldu, V, ldv, n_items, k, code, n, ms, _splits(splits), nrows


def topk_scores_for(h, users, U, V, n, min_score=None, splits=None):
    """
    topk_scores for a list of rows: (items int32 [m, n], scores float64 [m, n], counts int32 [m]) with m = len(users), row r
    of the result for row users[r] of U and of the handle's matrix.  users may be in any order and repeat a row.  The items
    are cut into `splits` ranges that run side by side (None: as many as fill the card), which changes no bit: for
    users = arange(b, e) the result is topk_scores' for rows = (b, e) (include/csrk.h, csrk_topk_scores_for).  Only the listed
    rows of U are sent.  Not a reference entry point.
    """
    users, U, ldu, V, ldv, n_items, k, code, n, ms, sp, nrows = topk_scores_for_args(h, users, U, V, n, min_score, splits)
    m = len(users)
    H = 0 if h is None else _live(h)
    lim = topk_scores_limits()
    if k > lim[0] or n > lim[1]:      # the library's refusal, before any result array is made
        one = np.zeros(1, np.int32)
        check(lib.csrk_topk_scores_for(H, ptr(one), 1, nrows, ptr(U), ldu, ptr(V), ldv, n_items, k, code, n, ms, None, n, None, n, None, sp))
        raise ValueError(f'k = {k} or n = {n} is above the limits {lim[:2]}')
    items, scores, counts = np.empty((m, n), np.int32), np.empty((m, n), np.float64), np.zeros(m, np.int32)
    if m == 0:
        return items, scores, counts
    _call(lib.csrk_topk_scores_for, H, ptr(users), m, nrows, ptr(U), ldu, ptr(V), ldv, n_items, k, code, n, ms, ptr(items), n, ptr(scores),
          n, ptr(counts), sp)
    return items, scores, counts


def rank_entries_limits():
    "(largest k, rows per workgroup, items per tile, factors per LDS chunk, test entries of a row per sweep)"
    return _limits(lib.csrk_rank_entries_limits, 5)


def rank_entries_args(seen_h, test_h, U, V, rows=None):
    """
    (U, ldu, V, ldv, k, panel code, row_begin, row_end) as the library takes them; ValueError for anything it would refuse
    as invalid.  test_h is anything with nrows and ncols (a handle or a CSR: the held-out pairs), seen_h the same (the
    pairs already seen) or None; no library call is made.
    """
    for name, h in (('test', test_h), ('seen', seen_h)):
        if h is None and name == 'seen':
            continue
        if isinstance(h, np.ndarray) or not all(hasattr(h, a) for a in ('nrows', 'ncols', 'nnz')):
            raise ValueError(f'{name} must be a CSR or a handle, not {type(h).__name__}')
    if seen_h is not None and (int(seen_h.nrows), int(seen_h.ncols)) != (int(test_h.nrows), int(test_h.ncols)):
        raise ValueError(f'seen is {seen_h.nrows} x {seen_h.ncols} but test is {test_h.nrows} x {test_h.ncols}')
    U, ldu, V, ldv, _, k, code, _, _, rb, re_ = topk_scores_args(test_h, U, V, 1, None, rows)
    return U, ldu, V, ldv, k, code, rb, re_


def rank_entries(seen_h, test_h, U, V, rows=None):
    """
    Offline evaluation of a factor model: for every entry (i, j) that test_h stores in rows = (begin, end) (None: all rows),
    in storage order, the number of items c != j that seen_h does not store in row i (None: no item is left out) and whose
    score dot(U[i, :], V[c, :]) comes before j's -- (ranks int32 [m], scores float64 [m]) with m the entries of those rows.
    Scores and order are topk_scores': one chain of k fused multiply-adds in float64, NaN above +Inf, -0.0 tied with +0.0,
    ties to the smaller item; an entry of rank r < n that seen_h does not store is topk_scores' items[i][r] (include/csrk.h,
    csrk_rank_entries).  seen_h's matrix must be canonical, test_h's need not be.  Not a reference entry point.
    """
    U, ldu, V, ldv, k, code, rb, re_ = rank_entries_args(seen_h, test_h, U, V, rows)
    sh = 0 if seen_h is None else _live(seen_h)
    lim = rank_entries_limits()
    if k > lim[0]:      # the library's refusal, before any result array is made
        check(lib.csrk_rank_entries(sh, _live(test_h), rb, re_, ptr(U), ldu, ptr(V), ldv, k, code, None, None))
        raise ValueError(f'k = {k} is above the limit {lim[0]}')
    m = 0
    if re_ > rb and test_h.nnz:
        m = row_extent(test_h, re_ - 1)[1] - row_extent(test_h, rb)[0]
    ranks, scores = _out(m, np.int32), _out(m, np.float64)
    _call(lib.csrk_rank_entries, sh, _live(test_h), rb, re_, ptr(U), ldu, ptr(V), ldv, k, code, ptr(ranks), ptr(scores))
    return ranks, scores


def rank_entries_for_limits():
    "(most splits, workgroups that fill the card)"
    return _limits(lib.csrk_rank_entries_for_limits, 2)


def rank_entries_for_splits(n_rows, n_items, splits=None):
    """
    Into how many ranges rank_entries_for cuts the items for n_rows listed rows and n_items items (splits=None: as many as
    fill the card).  From the library's constants alone: no device is touched.
    """
    for name, v in (('n_rows', n_rows), ('n_items', n_items)):
        if not _is_int(v):
            raise ValueError(f'{name} must be an integer, not {v!r}')
    if n_items > np.iinfo('i4').max:
        raise ValueError(f'{n_items} items are more than 32-bit indices hold')
    used = C.c_int32(0)
    check(lib.csrk_rank_entries_for_splits(int(n_rows), int(n_items), _splits(splits), C.byref(used)))
    return used.value


def rank_entries_for_args(seen_h, test_h, users, U, V, splits=None):
    """
    (users int32, U, ldu, V, ldv, k, panel code, splits, u_rows) as the library takes them; ValueError for anything it would
    refuse as invalid.  seen_h and test_h are as in rank_entries_args; users is a 1-D array of integer row indices in any
    order, repeats allowed; no library call is made.
    """
    U, ldu, V, ldv, k, code, _, nrows = rank_entries_args(seen_h, test_h, U, V, None)
    users = _row_list(users, nrows)
    return users, U, ldu, V, ldv, k, code, _splits(splits), nrows


def rank_entries_for(seen_h, test_h, users, U, V, splits=None):
    """
    rank_entries for a list of rows: (ranks int32 [m], scores float64 [m]) with m the entries test_h stores in the rows
    users[0], users[1], ... -- row by row in list order, each row's entries in storage order.  users may be in any order and
    repeat a row; every occurrence gets its own outputs.  The items are cut into `splits` ranges that run side by side (None:
    as many as fill the card) and the partial ranks add, which changes no bit: for users = arange(b, e) the result is
    rank_entries' for rows = (b, e) (include/csrk.h, csrk_rank_entries_for).  Only the listed rows of U are sent.  Not a
    reference entry point.
    """
    users, U, ldu, V, ldv, k, code, sp, nrows = rank_entries_for_args(seen_h, test_h, users, U, V, splits)
    sh = 0 if seen_h is None else _live(seen_h)
    lim = rank_entries_limits()
    if k > lim[0]:      # the library's refusal, before any result array is made
        one = np.zeros(1, np.int32)
        check(lib.csrk_rank_entries_for(sh, _live(test_h), ptr(one), 1, nrows, ptr(U), ldu, ptr(V), ldv, k, code, None, None, 0, sp))
        raise ValueError(f'k = {k} is above the limit {lim[0]}')
    m = 0
    if len(users) and test_h.nnz:
        m = int(row_nnzs(test_h)[users].sum(dtype=np.int64))
    ranks, scores = _out(m, np.int32), _out(m, np.float64)
    if m == 0:
        return ranks, scores
    _call(lib.csrk_rank_entries_for, sh, _live(test_h), ptr(users), len(users), nrows, ptr(U), ldu, ptr(V), ldv, k, code, ptr(ranks),
          ptr(scores), m, sp)
    return ranks, scores


_KNN_AGGREGATES = {'weighted-average': _lib.KNN_WEIGHTED_AVERAGE, 'sum': _lib.KNN_SUM}


def knn_scores_limits():
    """
    (lanes that share one target's walk, targets of a workgroup tile, entries of a rating row held in LDS, bits of the column
    filter, most tiles per workgroup, workgroups below which a workgroup takes one tile)
    """
    return _limits(lib.csrk_knn_scores_limits, 6)


def knn_scores_args(model, ratings, users, max_nbrs=0, min_nbrs=1, aggregate='weighted-average', offsets=None):
    """
    (users int32, max_nbrs, min_nbrs, aggregate code, offsets float64 or None) as the library takes them; ValueError for
    anything it would refuse as invalid.  model and ratings are anything with nrows and ncols (handles or CSRs); users is a
    1-D array of integer row indices of ratings in any order, repeats allowed; max_nbrs = 0 is no limit; offsets is None or
    one real number per user.  No library call is made.
    """
    if not isinstance(aggregate, str) or aggregate not in _KNN_AGGREGATES:
        raise ValueError(f"aggregate must be 'weighted-average' or 'sum', not {aggregate!r}")
    if not _is_int(max_nbrs) or max_nbrs < 0:
        raise ValueError(f'max_nbrs must be an integer that is not negative, not {max_nbrs!r}')
    if not _is_int(min_nbrs) or min_nbrs < 1:
        raise ValueError(f'min_nbrs must be an integer that is at least 1, not {min_nbrs!r}')
    if int(model.ncols) != int(ratings.ncols):
        raise ValueError(f'model is {model.nrows} x {model.ncols} but ratings is {ratings.nrows} x {ratings.ncols}: the columns differ')
    users = _row_list(users, int(ratings.nrows))
    if offsets is not None:
        offsets = np.asarray(offsets)
        if offsets.dtype == np.bool_ or not (np.issubdtype(offsets.dtype, np.floating) or np.issubdtype(offsets.dtype, np.integer)):
            raise ValueError(f'offsets must hold real numbers, not {offsets.dtype}')
        if offsets.shape != (len(users),):
            raise ValueError(f'offsets must hold one number per user ({len(users)}), not shape {offsets.shape}')
        offsets = np.ascontiguousarray(offsets, dtype=np.float64)
    i4 = np.iinfo('i4').max
    return users, min(int(max_nbrs), i4), min(int(min_nbrs), i4), _KNN_AGGREGATES[aggregate], offsets


_KNN_ROUTES = ('walk', 'reach')
KNN_STATS = ('reach', 'ranges_per_row', 'workgroups', 'count_from_marks', 'built_index', 'entries')
KNN_REACH_LIMITS = ('range', 'lanes', 'lds_row', 'filter_bits', 'round', 'chunk', 'long_reach_row')


def knn_route_arg(route):
    "route as given, or ValueError: 'walk' (every target of every listed row) or 'reach' (only the targets the user's ratings reach)"
    if not isinstance(route, str) or route not in _KNN_ROUTES:
        raise ValueError(f"route must be 'walk' or 'reach', not {route!r}")
    return route


def knn_scores(model_h, ratings_h, users, max_nbrs=0, min_nbrs=1, aggregate='weighted-average', offsets=None, route='walk'):
    """
    Scores from an item-kNN model on the device: NEW handle [len(users) x model.nrows], float64, canonical.  For user
    users[r] and each target i, the entries (j, s) of model row i are walked in storage order; those whose item j the user
    has rated (value v in ratings_h) are hits, the walk ends after max_nbrs hits (0: no limit), and target i is stored when
    it had at least min_nbrs hits: sum(v s) / sum(|s|) over the hits ('weighted-average') or sum(s) ('sum'), plus offsets[r]
    when offsets is given.  Every operation is rounded on its own, in storage order: the result is a function of its
    arguments, bit for bit (include/csrk.h, csrk_knn_scores).  ratings_h's matrix must be canonical, model_h's need not be.
    route='walk' visits every target for every user; route='reach' only the targets that hold one of the user's rated items
    (csrk_knn_scores_reach: the same bits; model_h keeps the index the route needs, knn_reach_index; the model's columns must
    lie in [0, ncols)).  Not a reference entry point.
    """
    fn = lib.csrk_knn_scores_reach if knn_route_arg(route) == 'reach' else lib.csrk_knn_scores
    users, mx, mn, code, offsets = knn_scores_args(model_h, ratings_h, users, max_nbrs, min_nbrs, aggregate, offsets)
    out = handle_t(0)
    _call(fn, _live(model_h), _live(ratings_h), ptr(users), users.size, mx, mn, code, ptr(offsets), C.byref(out))
    return _wrap(out.value)


def knn_reach_index(model_h, build=True):
    """
    (entries, device bytes) of the reach index model_h holds -- the structure-only transpose of the model's pattern that
    knn_scores(route='reach') marks its candidates from -- built first when build is true and there is none; (0, 0) when
    there is none and build is false.  The handle keeps it until order_columns or an in-place value operation drops it.
    """
    entries, nbytes = C.c_int64(0), C.c_int64(0)
    _call(lib.csrk_knn_reach_index, _live(model_h), 1 if build else 0, C.byref(entries), C.byref(nbytes))
    return int(entries.value), int(nbytes.value)


def knn_scores_reach_limits():
    """
    (targets of a range = bits of the mark bitmap, lanes that share a walk, entries of a rating row held in LDS, bits of the
    column filter, candidates walked per round, targets per enumeration chunk, longest reach row a group of lanes marks)
    """
    return _limits(lib.csrk_knn_scores_reach_limits, len(KNN_REACH_LIMITS))


def knn_scores_last_stats():
    """
    what this thread's last knn_scores did, as a tuple in KNN_STATS' order (include/csrk.h, csrk_knn_scores_last_stats): all
    zero after route='walk', after a call that failed and after an empty result
    """
    return _limits(lib.csrk_knn_scores_last_stats, len(KNN_STATS))


def set_spgemm_order(order):
    """
    Column order inside the rows mult_ab / mult_abt return: 'reference' (default) -- reverse order of first discovery,
    what csr/kernels/numba/multiply.py:79-82, 94-97 emit --, 'ascending' (the product kernels' own: no ordering pass) or
    None (follow CSRK_SPGEMM_ORDER: "ascending", else the reference's).  Process-wide, and followed by every route: the
    dense-panel route (a fully populated B, spgemm_last_route) too.  The values are the same bits either way.
    """
    code = {None: -1, 'ascending': 0, 'reference': 1}[order]
    check(lib.csrk_spgemm_set_order(code))


def spgemm_order():
    "the column order in force: 'reference' or 'ascending'"
    o = C.c_int(0)
    check(lib.csrk_spgemm_get_order(C.byref(o)))
    return 'reference' if o.value else 'ascending'


def spgemm_last_route():
    """
    what this thread's last mult_ab / mult_abt took: 'dense-panel' -- B was a fully populated CSR in row-major panel form
    (BASELINE configs[2] through the reference's own entry: csr/csr.py:524-567 -> multiply.py:13-38) -- or 'general'
    """
    r = C.c_int(0)
    check(lib.csrk_spgemm_last_route(C.byref(r)))
    return 'dense-panel' if r.value else 'general'


SPGEMM_STATS = ('general', 'fast', 'strips', 'strip_rows', 'strip_entries', 'strip_fused', 'esc_rows', 'esc_products', 'large_rows',
                'lds_symbolic', 'lds_rows', 'hash_big_rows', 'hbm_rows', 'small_fused', 'mid_rows', 'hash_rows')
SPGEMM_LIMITS = ('SG_WAVE_CAP', 'SG_CAP', 'SGE_MIN', 'SGE_TILE', 'SGS_W', 'SGS_MAX_S', 'SGS_MIN_PER_CELL', 'SGS_MIN_PER_UNIT',
                 'SGS_HEAVY_J', 'SGL_W', 'SGL_MAXTILES', 'SGL_MAXBITS', 'SGB_CAP', 'SG_COUNT_LONG', 'SG_COUNT_VLONG', 'SO_LEAST',
                 'SO_TINY', 'SO_WAVE', 'SO_MID', 'SO_WIN')


def spgemm_last_stats():
    """
    what the general product did with the rows of this thread's last mult_ab / mult_abt, as a dict (include/csrk.h,
    csrk_spgemm_last_stats): all zero after a call that failed or took the dense-panel route
    """
    out = (C.c_int64 * len(SPGEMM_STATS))()
    check(lib.csrk_spgemm_last_stats(out, len(SPGEMM_STATS)))
    return dict(zip(SPGEMM_STATS, (int(v) for v in out)))


def spgemm_limits():
    "the compile-time constants the general product routes its rows by, as a dict (include/csrk.h, csrk_spgemm_limits)"
    return dict(zip(SPGEMM_LIMITS, _limits(lib.csrk_spgemm_limits, len(SPGEMM_LIMITS))))


# csrk_spmv_plan_stats, slot by slot (include/csrk.h), and csrk_spmv_stream_limits
SPMV_PLAN_STATS = ('tiles', 'tile_items', 'cut_rows', 'path_entries', 't0_tiles', 't0_blocks', 't0_min', 't0_block_width', 'split_mode',
                   't0_rows', 't0_entries', 't1_rows', 't1_pairs', 't1_entries', 't1_min', 't1_block_width', 'n_hot', 'hot_cover_ppm',
                   't0_acc', 'hot_slots', 'stream', 'ls_tiles', 'ls_runs', 'ls_grid', 'ls_staged', 'plan_bytes', 'ls_round_tiles',
                   't0_workgroups', 'reserved', 'bytes_t0', 'bytes_t1', 'bytes_stream', 'bytes_staging', 'bytes_tables',
                   'ls_dense', 'ls_idx24', 'ls_hot_lds', 'ls_rounds', 'ls_wg_rounds', 'ls_stage_blocks', 'ls_stage_width', 'ls_f32',
                   't1_blocks', 't1_tiles', 't1_carry_rows', 't1_listed_carries', 't1_groups', 't1_pad_groups')
SPMV_STREAM_LIMITS = ('ACC_TILE', 'ACC_K', 'LS_WAVES', 'LS_SEQ', 'LS_RID', 'LS_HOT_LDS', 'LS_RND_HOT', 'LS_RND_CAP', 'LS_RND_MAXTILES',
                      'LS_STAGE_WMAX', 'LS_STAGE_BATCH', 'TIERB_MIN', 'HOT_SLOTS')


def spmv_plan_stats(h):
    "the handle's SpMV plan as a dict (include/csrk.h, csrk_spmv_plan_stats): builds the plan if the handle has none"
    out = (C.c_int64 * len(SPMV_PLAN_STATS))()
    check(lib.csrk_spmv_plan_stats(_live(h), out, len(SPMV_PLAN_STATS)))
    return dict(zip(SPMV_PLAN_STATS, (int(v) for v in out)))


def spmv_stream_limits():
    "the compile-time constants the light stream's form is decided by, as a dict (include/csrk.h, csrk_spmv_stream_limits)"
    return dict(zip(SPMV_STREAM_LIMITS, _limits(lib.csrk_spmv_stream_limits, len(SPMV_STREAM_LIMITS))))


def set_spmv_algo(h, name):
    "select the SpMV kernel for this handle: 'auto' | 'merge' | 'vector' | 'scalar'"
    code = {'auto': _lib.SPMV_AUTO, 'merge': _lib.SPMV_MERGE, 'vector': _lib.SPMV_VECTOR,
            'scalar': _lib.SPMV_SCALAR}[name]
    check(lib.csrk_set_spmv_algo(_live(h), code))


def device_count():
    n = C.c_int(0)
    check(lib.csrk_device_count(C.byref(n)))
    return n.value


def set_device(i):
    check(lib.csrk_set_device(int(i)))
