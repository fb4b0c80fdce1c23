"""Writes tests/golden/vs_ref_digests.json from the UNMODIFIED ETSI reference (oracle/_ref/liblc3_etsi_fl.so, built by oracle/Makefile
from the reference's sources): the md5 of the reference's outputs (and its API return codes) for every case of tests/test_oracle_vs_ref.py.
Run where oracle/_ref is built:  python tests/golden/make_golden_vs_ref.py.  Data only, no reference code."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_oracle_vs_ref as T  # noqa: E402
from lc3_harness import have_ref  # noqa: E402

assert have_ref(), "oracle/_ref is not built"
with open(T.DIGESTS, "w") as f:
    json.dump(dict(T.reference_cases()), f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", T.DIGESTS)
