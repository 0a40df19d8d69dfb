"""The route tier table (reporter_amd/csrc/otr_tiers.h) keeps the numbering the engine had in
literals: slot -> counter bank [0,2,3,4,5,6,8,9,7,1,10,11,12,13], list counter word, work
queue, dump-counter line and event pair, the other list counter words, and the
route_tier_code values; the retry protocol keeps the values the kernels and the engine had in
literals: every route and path flag, every collect's mask per slot and per path tier (node
tier t's for t = 0..4), edge_overflow_flag at 360 / 512 / 1024, the path tiers' sizes, grids,
counter words and queues, the run order, the OTR_FORCE_EDGE bits, and the task record word
through pack and accessors at the field extremes; and its OTR_TIERS parser gives the known answers (default list, at
most four tiers then 40961, unknown items dropped).  A stand-alone host program
(tests/route_tier_table_check.cpp) compares them; the header's static_asserts (ranges,
distinctness, every flag taken by a later tier or the left-over collect) are checked by compiling it."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = shutil.which('g++') or shutil.which('c++')


def test_route_tier_table_and_parser(tmp_path):
    assert CXX, 'no host C++ compiler found'
    exe = str(tmp_path / 'route_tier_table_check')
    subprocess.run([CXX, '-O1', '-std=c++17', '-Wall', '-I' + os.path.join(ROOT, 'reporter_amd', 'csrc'), '-o', exe,
                    os.path.join(HERE, 'route_tier_table_check.cpp')], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True)
    bad, checked = (int(x) for x in p.stdout.split())
    assert checked > 100, checked
    assert bad == 0, p.stderr
