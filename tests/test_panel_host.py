"""
csr_amd/csrc/panel.h on the host: the offsets and pitches of pack_panel / unpack_panel (rows = 0, a NULL source, a row
offset, padded strides), panel_rows_from, the 16-B predicate and mark_user_stream, in a small stand-alone program
(tests/panel_host/main.cpp) whose two HIP copies are memcpy stand-ins and whose pool is malloc of the exact size, built with
the build's compiler for the host only, without the HIP runtime, under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_and_unpack_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'panel_host')
    r = subprocess.run([os.environ.get('HIPCC', 'hipcc'), '--offload-arch=gfx950', '--cuda-host-only', '-no-hip-rt', '-std=c++17', '-O1',
                        '-g', '-Wall', '-Wno-unused-function', '-Werror', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                        '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'csr_amd', 'csrc'), os.path.join(ROOT, 'tests', 'panel_host', 'main.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'all cases passed' in r.stdout
