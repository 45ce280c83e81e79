"""
csr_amd/csrc/spmv_launch.h on the host: the decisions an SpMV product takes before it launches (spmv.hip, "host side";
DESIGN.md section 4, "The launch side") -- in a small stand-alone C++ program (tests/spmv_launch_host/main.cpp) built with
the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer.  The lazy split, the algorithm and its parts,
the light stream's form with its LDS and gather bases, tier 0's groups as launches, the rider's blocks and the epilogue's
jobs, order and batches are each held to values worked out by hand at their edges; a two-batch epilogue or a disagreement
between groups and launches needs a plan of eight groups, or a broken one, to show in a product on the device.  The header
must also compile on its own, without any device header.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'csr_amd', 'csrc')

CASES = ('split: forced by each of three variables', 'split: query or launch, first or second', 'split: open, and the rebuild',
         'algorithm: fewer than two entries', 'algorithm: parts', 'stream form: modes', 'stream form: LDS', 'stream form: bases',
         'stream form: float32 x read directly', 'tier 0: groups as launches', 'tier 0: groups and launches disagree',
         'tier 0: blocks, LDS and map of a launch', 'tier 0: value form', 'rider: when it rides', 'rider: blocks',
         'epilogue: blocks of a fix, a reduce, a scatter', "epilogue: tier 0's and tier 1's jobs",
         'epilogue: order fix, tier 0, tier 1', 'epilogue: batches of six', 'epilogue: empty jobs are skipped',
         'epilogue: a failed launch')


def test_spmv_launch_header_is_plain_cxx(tmp_path):
    tu = tmp_path / 'only_the_header.cpp'
    tu.write_text('#include "spmv_launch.h"\nint main() { return 0; }\n')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-I', CSRC, str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_spmv_launch_decisions_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'spmv_launch_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', CSRC,
                        os.path.join(ROOT, 'tests', 'spmv_launch_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    for case in CASES:
        assert f'ok   {case}' in r.stdout, case
