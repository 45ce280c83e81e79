"""
The 8.5-byte entries of tier 0's stream on the host (csr_amd/csrc/fix56.h, namespace nib): 6.5-byte
values in three planes -- the mantissa's top nibble in a 4-bit plane -- beside a 16-bit index word {sign, row step, 12-bit
column}, "sign set, mantissa 0" meaning a padding entry.  A small stand-alone C++ program (tests/nib_host/main.cpp), built
with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer, sends every slot of a tile through encode,
put, get and the decode the product kernel runs: value bits, column and step must come back, a padding entry as -0.0 on
the window's zero slot.  It also checks the arithmetic of the rule that selects the form (accgroups::choose_nib).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nib_roundtrip_and_selection_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'nib_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'nib_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    assert 'FAIL' not in r.stdout
    for case in ('random grid, g = -52', 'random grid, g = -1074', 'random grid, g = 971', 'extremes', 'zeros and padding',
                 'sign and nibble only', 'sign and one plane only', 'padding only', 'rule: unset, 16 tiles per workgroup',
                 'rule: unset, one entry short', 'rule: knob 1, small', 'rule: knob 0, large'):
        assert f'ok   {case}' in r.stdout, case
