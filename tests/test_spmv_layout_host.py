"""
csr_amd/csrc/spmv_layout.h on the host: the arithmetic that lays an SpMV plan out (spmv_plan.hip, "host side"; DESIGN.md
section 4, "The plan builder") and the parsing of the plan's knobs -- in a small stand-alone C++ program
(tests/spmv_layout_host/main.cpp) built with the system compiler under AddressSanitizer and UndefinedBehaviorSanitizer.
Tile starts, the tier-1 workgroup list and carry slots, tier 0's tasks, shares, segments and threshold, the pack's threshold,
the staging blocks and rounds and the size rules are each held to values worked out by hand at their edges; several of
those edges need rows of 2^16 entries, 256 compute units or 2^31 entries to show in a product on the device.  The header
must also compile on its own, without any device header.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'csr_amd', 'csrc')

CASES = ('structures', 'knobs: nothing set', 'knobs: CSRK_HEAVY_MIN', 'knobs: CSRK_TIERB_MIN', 'knobs: CSRK_ACC_GROUPS',
         'knobs: CSRK_ACC_GROUP_ROWS', 'knobs: CSRK_SPMV_NIB', 'knobs: switches', 'size rules', 'tier1_pairs_fit',
         'free-memory predicates', 'dense_rows_pay', 'tile_starts', 'panel_groups: 15 blocks, plain',
         'panel_groups: 16 blocks, streams and pads', 'panel_groups: xcd_streams off', 'panel_carries: 0, 4 and 5 carries',
         'panel_carries: listed in tile order', 'panel_carries: nothing listed', 'acc_tasks', 'wg_shares', 'acc_segments',
         'acc_lds_bytes', 'tier0_threshold: no extension', 'tier0_threshold: kth in the histogram',
         'tier0_threshold: kth beyond the histogram', 'tier0_threshold: ties', 'tier0_threshold: floor',
         'tier0_threshold: n_cut below the capacity', 'tier0_threshold: never raised', 'split_rows',
         'hot threshold: top bin above the cap', 'hot threshold: everything fits',
         'hot threshold: stops at the bin that would overflow', 'stage_blocks', 'stage_rounds', 'next_round_size')


def test_spmv_layout_header_is_plain_cxx(tmp_path):
    tu = tmp_path / 'only_the_header.cpp'
    tu.write_text('#include "spmv_layout.h"\nint main() { return 0; }\n')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-I', CSRC, str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_spmv_layout_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'spmv_layout_host')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=all', '-I', CSRC,
                        os.path.join(ROOT, 'tests', 'spmv_layout_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
    for case in CASES:
        assert f'ok   {case}' in r.stdout, case
