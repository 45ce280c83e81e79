"""
csr_amd/csrc/score_plan.h on the host: what the four factor-score drivers decide (topk_scores.hip, topk_scores_for.hip,
rank_entries.hip, rank_entries_for.hip; DESIGN.md sections 8d-8i, "The drivers") in a small stand-alone C++ program
(tests/score_plan_host/main.cpp) built with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer and
run as a child process.
  1. Every function of the header at its edges, the expected values worked out by hand from rules 4 and 11 of
     include/csrk.h.
  2. The request grids of test_topk_scores_for_host.py's rule-4 test and test_rank_entries_for_host.py's rule-11 test through
     the program's `case` mode: the header's splits and bytes must equal tests/score_rules.py's restatement -- the text those
     two tests compare the library with.
"""
import os
import subprocess

import pytest

import score_rules as RULES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGES = ('constants', 'the knob parser', 'limits and list classes', 'the wide rule', 'row blocks', 'rule 11 over the rows',
         'rule 4 over the rows, n_top <= 32', 'rule 4 over the rows, n_top > 32', 'tile counts', 'forced splits', 'workspace bytes',
         'the two grid limits', 'the capped grids', 'item ranges')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('score_plan_host') / 'score_plan_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'score_plan_host', 'main.cpp'), '-o', path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path


def test_score_plan_edges_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    lines = r.stdout.splitlines()
    for case in EDGES:
        assert f'ok   {case}' in lines, case
    assert len([ln for ln in lines if ln.startswith('ok   ')]) == len(EDGES)


def _answers(exe, requests):
    r = subprocess.run([exe, 'case'], input='\n'.join(requests) + '\n', capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(requests)
    return out


def test_the_header_follows_rule_4(exe):
    from csr_amd.kernels import hip as K
    lim, tlim = K.topk_scores_for_limits(), K.topk_scores_limits()
    reqs = [(n_rows, n_items, n, splits) for n in RULES.RULE4_NS for n_rows, n_items, splits in RULES.rule4_grid(n, lim)]
    got = _answers(exe, [f'4 {n_rows} {n_items} {n} {splits or 0}' for n_rows, n_items, n, splits in reqs])
    assert len(reqs) == 6 * 7 * 7 * 8
    for (n_rows, n_items, n, splits), g in zip(reqs, got):
        assert g == RULES.rule4(n_rows, n_items, n, splits, lim, tlim), (n_rows, n_items, n, splits, g)
    assert {1, 2, 3, 5, lim[0]} <= {g[0] for g in got}
    # not vacuous for the round-up: some request's slots are no multiple of 16 bytes
    assert any(g[0] > 1 and (r[0] * g[0] * (lim[3] + lim[4] * (r[2] - 1))) % 16 for r, g in zip(reqs, got))


def test_the_header_follows_rule_11(exe):
    from csr_amd.kernels import hip as K
    (s_max, W), rlim = K.rank_entries_for_limits(), K.rank_entries_limits()
    block, tile = rlim[1], rlim[2]
    reqs = list(RULES.rule11_grid(s_max, W, tile))
    got = _answers(exe, [f'11 {n_rows} {n_items} {splits or 0}' for n_rows, n_items, splits, _ in reqs])
    assert len(reqs) == 8 * 7 * 9
    for (n_rows, n_items, splits, T), g in zip(reqs, got):
        assert g == (RULES.rule11(n_rows, n_items, splits, s_max, W, block, tile),), (n_rows, n_items, splits, g)
    assert {1, 2, 3, 5, s_max} <= {g[0] for g in got}
