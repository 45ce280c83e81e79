"""
csr_amd/csrc/spgemm_plan.h on the host: the decisions of the general sparse product's driver (spgemm.hip, "the driver";
DESIGN.md section 8) -- the strips in force, when the sub-range table pays, when the expand-sort-compress products fit the
sort's budget and free memory, the one-pass forms' temporaries, the dense path's grid, the sizes of the driver's scratch --
in a small stand-alone C++ program (tests/spgemm_plan_host/main.cpp) built with the system compiler under AddressSanitizer
and UndefinedBehaviorSanitizer.  Every rule is asked at its edge, with expected values worked out by hand: the budgets
(2 GiB, 200 Mi products, 6 and 24 GiB) are beyond any input the GPU tests can afford, so the fallbacks that
tests/spgemm_cases.py lists as "not covered" on the device are checked here.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spgemm_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'spgemm_plan_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'spgemm_plan_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    for case in ('constants', 'strips in force', 's_dense', 'the sub-range table pays', "the ESC products fit the sort's budget",
                 'the ESC products fit free memory', 'hash_rows and mid_rows', 'small_fused', 'strip_fused', 'grid_dense',
                 'scratch_len', 'long_cap and the size of list_s'):
        assert f'ok   {case}' in r.stdout, case
