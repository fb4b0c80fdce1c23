"""Writes tests/golden/quiet_tails_sha256.json: one SHA-256 per (family, class) of the PCM of tests/quiet_tails.py (test_quiet_tails_cpu.py pins it)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quiet_tails as qt

out = {}
for fam in qt.FAMILIES:
    pcm, names = qt.enc_streams(fam)
    for k, x in zip(names, pcm):
        out["%s/%s" % (qt.fam_id(fam), k)] = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
with open(os.path.join(HERE, "quiet_tails_sha256.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
