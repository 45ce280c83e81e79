"""
csr_amd/csrc/acc_groups.h on the host: how SpMV's tier 0 deals its rows to groups and launches, splits the compute units
between the groups of one launch and places their workgroups on the launch's blocks -- in a small
stand-alone C++ program (tests/acc_groups_host/main.cpp) built with the system compiler under AddressSanitizer and
UndefinedBehaviorSanitizer.  Every row must land in exactly one group, every (group, workgroup) on exactly one block, and
the workgroups of one column range on blocks that are equal mod 8.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_acc_groups_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'acc_groups_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'acc_groups_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    for case in ('one group, as ever', 'G = 3, cap 41: exactly full', 'G = 3, cap 40: 120 + 3', 'G = 2, cap 61: 122 + 1',
                 'headline-sized', '256 CUs, 2 groups', '256 CUs, 3 groups', 'uneven groups 128 + 5 + 1',
                 '2 groups, long segments', '2 groups, short segments', '3 groups asked, 2 pay', 'rows below the floor'):
        assert f'ok   {case}' in r.stdout, case
