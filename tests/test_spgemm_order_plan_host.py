"""
csr_amd/csrc/spgemm_order_plan.h on the host: the decisions of the ordering pass's driver (spgemm_order.hip:
spgemm_apply_reference_order; DESIGN.md section 6, "The ordering pass's driver") in a small stand-alone C++ program
(tests/spgemm_order_plan_host/main.cpp) built with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer
and run as a child process.
  1. Every function of the header at its edges, the expected values worked out by hand: the LDS budget where the device's
     limit and the cap meet, the by-column window ladder at each rung's last column count, cols_mode at 2^32 - 1 entries of B,
     the by-entry capacity, the refusal on a device of 64 KiB and the smallest device that passes, the tiers for a row in
     every octave and at every boundary, the grids up to 2^31 - 1 rows, the byte sizes, the knob.
  2. Every case of tests/spgemm_cases.py: the header's LDS plan and tiers for the case's product (products and entries per
     row of C, columns, entries of the right operand) must be those of spgemm_cases.order_plan -- the NumPy-side statement --
     at the MI355X's LDS limit, and the cases together must reach every tier and every form of the 1024-thread walk.
"""
import os
import subprocess

import pytest

import spgemm_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGES = ('constants', 'the tier exponents', 'the static tables', 'the budget', 'the window ladder',
         'cols_mode at 2^32 - 1 entries of B', 'by entry, and the 256-thread walk', 'ok, and a 64 KiB device', 'tiers: no row',
         'tiers: a row in every octave', 'tiers: the boundaries, the flag, 2^31 - 1 rows', 'what the call starts from', 'the grids',
         'the byte sizes', 'the knob')

LDS = ('budget', 'by_col', 'win_cols', 'cols_mode', 'win_long', 'cap_long', 'lds_long', 'win_mid', 'cap_mid', 'lds_mid', 'lds_place', 'ok')
TIERS = ('listed', 'n_long', 'n_mid', 'n_wave', 'n_small', 'keys_in_memory')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('spgemm_order_plan_host') / 'spgemm_order_plan_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'spgemm_order_plan_host', 'main.cpp'), '-o', path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path


def test_order_plan_edges_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    lines = r.stdout.splitlines()
    for case in EDGES:
        assert f'ok   {case}' in lines, case
    assert len([ln for ln in lines if ln.startswith('ok   ')]) == len(EDGES)


def _program_plan(exe, c, lds_max):
    "the program's answer for a case: {line's first word: its integers}"
    rows = ''.join(f'{int(u)} {int(n)}\n' for u, n in zip(c.p.u, c.p.cnt))
    r = subprocess.run([exe, 'case', str(lds_max), str(c.r.ncols), str(c.r.nnz)], input=rows, capture_output=True, text=True)
    assert r.returncode == 0, (c.name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        key, *rest = line.split()
        out[key] = [int(v) for v in rest]
    assert set(out) == {'constants', 'lds', 'tiers', 'cursors'}, (c.name, sorted(out))
    return out


@pytest.mark.parametrize('name', S.names())
def test_the_header_plans_the_case_as_the_module_does(exe, name):
    c = S.build(name)
    want = S.order_plan(c, S.ORDER_LDS_MAX)
    got = _program_plan(exe, c, S.ORDER_LDS_MAX)
    L = S.LIMITS
    assert got['constants'] == [L['SO_LEAST'], L['SO_TINY'], L['SO_WAVE'], L['SO_MID'], L['SO_WIN'], S.SO_LDS_BYTES, S.SO_TABLES_BYTES,
                                S.SO_WIN_ENTRY], (name, got['constants'])
    assert dict(zip(LDS, got['lds'])) == {k: want[k] for k in LDS}, name
    assert dict(zip(TIERS, got['tiers'])) == {k: want[k] for k in TIERS}, name
    assert got['cursors'] == want['cursors'] + [want['keys_in_memory']], name
    assert want['ok'] == 1 and want['listed'] + want['n_least'] == int((c.p.u > 0).sum()), name


def test_the_cases_reach_every_tier_and_every_form_of_the_long_walk():
    "the comparison above is not vacuous: each tier has rows somewhere, and the long rows take each of their three forms"
    tiers, forms, place = set(), set(), False
    for name in S.CASES:
        p = S.order_plan(S.build(name))
        tiers |= {k for k in ('n_least', 'n_small', 'n_wave', 'n_mid', 'n_long') if p[k]}
        forms |= p['long_forms']
        place |= p['place']
    assert tiers == {'n_least', 'n_small', 'n_wave', 'n_mid', 'n_long'}
    assert forms == {'by column', 'by entry in LDS', 'in memory'} and place


def test_order_plan_by_hand():
    "the restatement on the two cases written for the pass, and away from the MI355X's limit"
    t = S.order_plan(S.build('order-tiers'))
    assert (t['n_least'], t['n_small'], t['n_wave'], t['n_mid'], t['n_long']) == (1, 2, 2, 2, 1)
    assert t['long_forms'] == {'by column'} and t['win_long'] == 8192 and t['lds_long'] == 4 * (5000 + 2 * 157) + 65536 and not t['place']
    w = S.order_plan(S.build('order-window'))
    assert (w['cols_mode'], w['cap_long'], w['lds_long']) == (0, 16128, 145408) and w['long_forms'] == {'in memory'} and w['place']
    assert (w['n_long'], w['n_small'], w['listed']) == (1, 1, 2)
    # 160768 columns: by entry; 20096 and 20095 entries are more than the 16128 LDS holds, 4097 and 4096 fit; 1024 products are a mid row
    f = S.order_plan(S.build('fb-160768'))
    assert f['cols_mode'] == 0 and f['long_forms'] == {'in memory', 'by entry in LDS'} and (f['n_long'], f['n_mid'], f['n_wave']) == (4, 1, 0)
    s = S.order_plan(S.build('order-window'), lds_max=65536)
    assert (s['budget'], s['cap_long'], s['ok']) == (47104, 3840, 0)
