"""
csr_amd/csrc/score_host.h on the host: the listed-rows steps of csrk_topk_scores_for and csrk_rank_entries_for --
check_listed_rows at -1, 0, u_rows - 1 and u_rows; pack_listed_rows for both element sizes, k = 1, 3, 4, packed and padded
strides and the lists (), (row) and (last, 0, last), with U and the packed copy allocated at exactly their sizes -- and the
other shared steps (the optional handle, the seen / test agreement, the canonical check with its lock, the refusal texts that
take the entry's name, the panel-type ladder), in a small stand-alone program (tests/score_host_host/main.cpp) whose HIP copy
is a memcpy stand-in and whose pool is malloc of the exact size, built with the build's compiler for the host only, without
the HIP runtime, under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_listed_rows_and_shared_steps_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'score_host_host')
    r = subprocess.run([os.environ.get('HIPCC', 'hipcc'), '--offload-arch=gfx950', '--cuda-host-only', '-no-hip-rt', '-std=c++17', '-O1',
                        '-g', '-Wall', '-Wno-unused-function', '-Werror', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                        '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'csr_amd', 'csrc'), os.path.join(ROOT, 'tests', 'score_host_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
