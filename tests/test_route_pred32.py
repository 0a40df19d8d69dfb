"""The node search's per-round predicates run in 32-bit arithmetic where the label words are
32 bits wide (reporter_amd/csrc/otr_pred.h: the IN criterion of the partition and the
target test).  A stand-alone host program (tests/route_pred32_check.cpp) compares them with
the 64-bit expressions they replaced: lengths and kmin at 0, 1, gap - 1, gap, 2^31 - 1,
2^31, 2^32 - 2, 2^32 - 1 (each +-1), gaps 1, 16 and 65535 * 16, partial lengths and bounds up
to 2^31 - 1, a target without a label, kmin = 0xFFFFFFFF, and a few million random tuples."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def test_pred32_equals_64bit_forms(tmp_path):
    # (the header is a HIP host/device header; the project does not build without hipcc either)
    assert os.path.exists(HIPCC), 'hipcc not found: the project needs ROCm to build'
    exe = str(tmp_path / 'route_pred32_check')
    subprocess.run([HIPCC, '-x', 'hip', '--cuda-host-only', '-O2', '-std=c++17',
                    '-I' + os.path.join(ROOT, 'reporter_amd', 'csrc'), '-o', exe,
                    os.path.join(HERE, 'route_pred32_check.cpp')], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split()
    bad, checked = int(out[0]), int(out[1])
    assert checked > 4000000, checked
    assert bad == 0, '%d of %d predicate results differ from the 64-bit forms' % (bad, checked)
