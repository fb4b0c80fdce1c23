"""Writes tests/golden/size_sweep_digests.json from the UNMODIFIED ETSI reference (oracle/_ref/liblc3_etsi_fl.so, built by oracle/Makefile from the
reference's sources): per family and block of 16 frame sizes the md5 of the reference encoder's frames and of the reference decoder's PCM and status on those
frames damaged (tests/test_size_sweep_cpu.py, tests/size_sweep.py), and in the header how many frames the portable-math oracle encodes differently from the
exact-math one on this machine.  Run where oracle/_ref is built:  python tests/golden/make_golden_size_sweep.py.  Data only, no reference code."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_size_sweep_cpu as M  # noqa: E402
from lc3_harness import have_ref  # noqa: E402

assert have_ref(), "oracle/_ref is not built"
with open(M.DIGESTS, "w") as f:
    json.dump(dict(M.reference_cases()), f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", M.DIGESTS)
