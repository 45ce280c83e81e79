"""
csr_amd/csrc/spmm_plan.h on the host: the decisions of the dense-panel SpMM's plan builder and launch side
(spmm_dense.hip; DESIGN.md section 7, "The plan builder and launch side") in a small stand-alone C++ program
(tests/spmm_plan_host/main.cpp) built with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer and
run as a child process.
  1. Every function of the header at its edges, the expected values worked out by hand.
  2. Every case of tests/spmm_cases.py at its first width, under its own environment, for 256, 8 and 100 compute units: the
     program takes the matrix through the header's functions in the builder's order and its nine statistics, R, range
     table, heavy rows and their group / wavefront / slot must equal spmm_cases.Plan -- the NumPy statement of the same
     plan, which tests/test_gpu_spmm_edges.py compares with the library on the device.
"""
import os
import subprocess

import numpy as np
import pytest

import spmm_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (256, 8, 100)           # MI355X; one XCD's worth and fewer than some cases have tiles; no multiple of 8

EDGES = ('constants', 'the knob parser', 'engage at 64 MiB', 'candidates', 'the pays rule', 'the forced first group',
         'HEAVY_GROUPS larger than the candidates allow', 'ties that fit', 'ties that move the threshold',
         'ties that switch the form off', 'shrink from 3 groups to 1', 'n_tiles', 'R at cus < G', 'R at 7, 8, 9, 15, 16 tiles',
         'the bucket limit at 2^30', '8 n_buckets against 12 nnz_h', 'the free-memory refusal', 'place codes', 'entry offsets',
         'balance_ranges at a goal met exactly', 'balance_ranges: the clamp low', 'balance_ranges: the clamp high',
         'balance_ranges with R == n_tiles', 'light_segments', 'full4 and hrows_even', 'column blocks', 'the three grids',
         'grow_partials', 'the nine stats with the heavy form off', 'the dense-B gate', 'c_nnz at INT32_MAX', 'choose_heavy')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('spmm_plan_host') / 'spmm_plan_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'spmm_plan_host', 'main.cpp'), '-o', path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path


def test_spmm_plan_edges_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    lines = r.stdout.splitlines()
    for case in EDGES:
        assert f'ok   {case}' in lines, case
    assert len([ln for ln in lines if ln.startswith('ok   ')]) == len(EDGES)


def _knob(v):
    return '-' if v is None else '=' + v


def _program_plans(exe, c, k):
    "the program's output for a case at width k: {cus: {key: list of int | str}}"
    env = c.env()
    text = '\n'.join([f'{c.ncols} {k} {len(CUS)} ' + ' '.join(map(str, CUS)),
                      ' '.join(_knob(env.get(key)) for key in T.ENV_KEYS) + ' - -',
                      f'{c.nrows} {c.nnz}', ' '.join(map(str, c.rowptrs.tolist())), ' '.join(map(str, c.colinds.tolist())), ''])
    r = subprocess.run([exe, 'case'], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (c.name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        key, *rest = line.split()
        if key == 'cus':
            cur = out.setdefault(int(rest[0]), {})
        elif key == 'tie':
            cur[key] = rest[0]
        else:
            cur[key] = [int(v) for v in rest]
    return out


@pytest.mark.parametrize('name', T.names())
def test_the_header_builds_the_models_plan(exe, name):
    c = T.build(name)
    k = c.ks[0]
    got = _program_plans(exe, c, k)
    assert sorted(got) == sorted(CUS)
    for cus in CUS:
        p, g = c.plan(cus, k), got[cus]
        what = (name, k, cus)
        assert g['stats'] == p.stats(), (what, dict(zip(T.STAT_KEYS, zip(g['stats'], p.stats()))))
        assert g['R'] == [p.R] and g['range'] == p.range.tolist(), (what, g['R'], p.R, g['range'], p.range.tolist())
        assert g['rows'] == p.rows.tolist(), what
        if p.on:
            assert (g['group'], g['wave'], g['slot']) == (p.group.tolist(), p.wave.tolist(), p.slot.tolist()), what
            assert g['tie'] == p.tie and g['G_taken'] == [p.G_before_shrink], (what, g['tie'], p.tie)
            assert len(g['range']) == p.R + 1 and np.all(np.diff(g['range']) >= 1) and g['range'][-1] == p.tiles, what
        else:
            assert g['group'] == g['wave'] == g['slot'] == [] and g['tie'] == '-', what


def test_the_cases_reach_both_sides_of_the_plan():
    "the comparison above is not vacuous: plans on and off, several groups, both mappings, both tie rules, at every CU count"
    for cus in CUS:
        plans = [T.build(n).plan(cus) for n in T.names()]
        assert {p.on for p in plans} == {True, False}
        assert {p.G for p in plans} >= {0, 1, 2, 3} and {p.tie for p in plans if p.on} == {'fit', 'move'}
        assert {p.by_xcd() for p in plans if p.on} == {True, False}
        assert any(p.on and p.R < p.tiles for p in plans) and any(p.on and p.R == p.tiles for p in plans)
