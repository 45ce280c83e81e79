"""
csr_amd/csrc/fix56.h on the host: the 7-byte form of grid-aligned float64 values -- the grid test,
encode, the three planes of a tile and the decode the product kernel runs -- in a small stand-alone C++ program
(tests/fix56_host/main.cpp) built with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer.  Every
value must come back bit for bit; the sets that must not pack are the ones with a NaN, an Inf, a -0.0, a value off the
grid, a mantissa of 2^52 or more, or a grid whose magic constant 2^(52 + g) is no normal number.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fix56_roundtrip_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'fix56_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'csr_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'fix56_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    for case in ('j * 2^-52', 'M = 2^52 - 1', 'M = 2^52', 'all zeros', 'one -0.0', 'one NaN', 'one Inf', '1/3 among grid values',
                 'subnormal grid', 'huge grid, g = 971', 'g = 972'):
        assert f'ok   {case}' in r.stdout, case
