"""
csr_amd/csrc/radix_plan.h on the host: the decisions of the stable radix sort's driver (transpose.hip: sort_records;
DESIGN.md section 5, "The driver") in a small stand-alone C++ program (tests/radix_plan_host/main.cpp) built with the system
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.
  1. Every function of the header at its edges, the expected values worked out by hand: the key-range ladder, the payload
     range at 2^24, n = 0, record counts around a chunk, the histogram's four chunks, the scatter grid's eight and the table
     scan's trip, the pass schedules, and which buffers each route requests.
  2. Every case of tests/radix_cases.py: the route the header takes for the case's (op, nrows, ncols, n) must be the one the
     case is meant for (Case.expect, which radix_cases.route -- the NumPy-side statement -- vouches for in the case's
     preconditions), the descriptors of the packed route must hold the aligned chunks the case's keys need, and the
     constants radix_cases restates must be the header's.
"""
import os
import subprocess

import numpy as np
import pytest

import radix_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGES = ('constants', 'the key-range ladder', 'the payload range at 2^24', 'n = 0', 'record counts 1 .. 8192 * 4096 + 1',
         'the size functions', 'the grids', 'the pass schedule', 'which buffers exist')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('radix_plan_host') / 'radix_plan_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'radix_plan_host', 'main.cpp'), '-o', path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path


def test_radix_plan_edges_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    lines = r.stdout.splitlines()
    for case in EDGES:
        assert f'ok   {case}' in lines, case
    assert len([ln for ln in lines if ln.startswith('ok   ')]) == len(EDGES)


def _program_sorts(exe, c):
    "the program's answer for a case: (constants, [(route, chunks, descriptor capacity) per sort])"
    r = subprocess.run([exe, 'case', c.op, str(c.nrows), str(c.ncols), str(c.n)], capture_output=True, text=True)
    assert r.returncode == 0, (c.name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    consts, sorts = None, []
    for line in r.stdout.splitlines():
        key, *rest = line.split()
        if key == 'constants':
            consts = tuple(int(v) for v in rest)
        else:
            assert key == 'sort', line
            sorts.append((rest[0], int(rest[1]), int(rest[2])))
    return consts, sorts


def _sort_keys(c):
    "the keys of each sort the case makes, in order"
    if c.op != 'order':
        return [c.keys()]
    # the second transpose sorts the first one's result by ITS columns: the source rows
    return [c.colinds, np.repeat(np.arange(c.nrows, dtype=np.int32), np.diff(c.rowptrs))]


@pytest.mark.parametrize('name', R.names())
def test_the_header_takes_the_route_the_case_is_meant_for(exe, name):
    c = R.build(name)
    consts, sorts = _program_sorts(exe, c)
    assert consts == (R.CHUNK, R.HIST_GROUP, R.SCAN_TRIP), (name, consts)
    routes = tuple(s[0] for s in sorts)
    assert (routes if c.op == 'order' else routes[0]) == c.expect and len(sorts) == (2 if c.op == 'order' else 1), (name, routes, c.expect)
    for (route, chunks, capacity), keys in zip(sorts, _sort_keys(c)):
        assert chunks == R.plain_chunks(c.n), (name, chunks)
        if route == 'packed':
            assert R.aligned_chunks(keys) <= capacity == chunks + 256, (name, R.aligned_chunks(keys), capacity)


def test_the_cases_reach_every_route_and_the_descriptor_limit():
    "the comparison above is not vacuous: every route but the empty one is expected somewhere, and one case fills the descriptors"
    expected = set()
    for name in R.names():
        if name != 'F-many-chunks':                   # (3.4e7 records to build; it is a one-pass case like others)
            e = R.build(name).expect
            expected |= set(e) if isinstance(e, tuple) else {e}
    assert expected == {'1', 'packed', 'plain2', '3', '4'}
    c = R.build('D-c-most-descriptors')
    assert R.aligned_chunks(c.keys()) == R.plain_chunks(c.n) + 255
