"""Repeat-run parity of the tuned forward kernels at many tiles per workgroup (tools/stress_parity.py with BATCH=64, REPS=2): every
element of every launch against the oracle.  An intermittent fault — like round 4's 16-byte store hazard, which showed only at >= 64 x 10 s
and only now and then — fails this test, not just a tool.  The criterion here is whole-batch (2e-4 max|ref|); tests/test_tile_walks.py holds the
same many-tile regimes, the inverse kernels included, to per-frame bounds and to bit equality with one-tile launches."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_tuned_forward_kernels_repeat_parity():
    env = dict(os.environ, BATCH="64", REPS="2", FORWARD_ONLY="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_parity.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, r.stdout[-3000:]
