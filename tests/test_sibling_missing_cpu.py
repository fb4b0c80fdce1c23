"""A missing sibling library (DESIGN.md "Sibling libraries") on the host alone, through the stub build (tools/stub_shim.c): audio_codec_amd/_stub/ holds the host
code and none of the six kernel libraries, and with lc3stub_device_args(1) a call gets as far as looking for its library.  Every entry point that needs a sibling
then returns LC3_ERROR, and stderr names each of the six files once, however often a call is repeated.  Run in a child process: a library is looked for once per
process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
STUB_DIR = os.path.join(ROOT, "audio_codec_amd", "_stub")
LC3_ERROR = 1
SIBLINGS = ["liblc3plus_%s_hip.so" % n for n in ("probe", "ingest", "egress", "rtp", "rtcp", "srtp")]
CALLS = ["probe", "ingest", "enc_egress", "dec_egress", "rtp_parse", "enc_rtp_stamp", "dec_rtp_stamp", "rtcp_stats", "enc_srtp_protect", "dec_srtp_protect",
         "srtp_unprotect"]

# every array argument is the same 64 zero bytes (the SRTP destination and the workspaces another block): the calls pass their checks and read none of them
CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, %(root)r)
import audio_codec_amd
from audio_codec_amd import api
L = audio_codec_amd.load_library()
a, d = (C.c_uint64 * 8)(), (C.c_uint64 * 64)()
A, D = C.addressof(a), C.addressof(d)
L.lc3stub_reset()
enc, dec = C.c_void_p(), C.c_void_p()
assert L.lc3plus_enc_batch_create(C.byref(enc), 1, 48000, 1, 10.0, 0, (C.c_int * 1)(64000), 0) == 0
assert L.lc3plus_dec_batch_create(C.byref(dec), 1, 48000, 1, 10.0, 0, (C.c_int * 1)(80), 0) == 0
egress = [1, A, 64, A, A, 40, A, 0, A, 1, A, A, 16, api.PACK_STREAM_MAJOR, A, 64, 0, 1] + [A] * 11 + [A, None, 1]
stamp = [1] + [A] * 7 + [1, 1, A, A, A, 480, api.RTP_MARKER_NEVER, A, A, A, A, 64, 12, 0, A, A, A, None, 1]
protect = [1] + [A] * 6 + [64, 12, 0, 1] + [A] * 4 + [D, 64, 32, 10] + [A] * 4 + [None, 1]
calls = {
    "probe": lambda: L.lc3plus_dec_batch_probe(dec, A, 64, A, A, 40, 1, api.PROBE_SIDE, A, None, 1),
    "ingest": lambda: L.lc3plus_dec_batch_ingest(dec, 1, *([A] * 7 + [16, 1] + [A] * 7 + [None, 1])),
    "enc_egress": lambda: L.lc3plus_enc_batch_egress(enc, *egress),
    "dec_egress": lambda: L.lc3plus_dec_batch_egress(dec, *egress),
    "rtp_parse": lambda: L.lc3plus_dec_batch_rtp_parse(dec, 1, A, 64, A, A, 1, A, A, A, 0, *([A] * 8 + [None, 1])),
    "enc_rtp_stamp": lambda: L.lc3plus_enc_batch_rtp_stamp(enc, *stamp),
    "dec_rtp_stamp": lambda: L.lc3plus_dec_batch_rtp_stamp(dec, *stamp),
    "rtcp_stats": lambda: L.lc3plus_dec_batch_rtcp_stats(dec, 1, A, A, A, A, 1, A, A, 0, *([A] * 7 + [D, L.lc3plus_rtcp_workspace_bytes(1, 1), None, 1])),
    "enc_srtp_protect": lambda: L.lc3plus_enc_batch_srtp_protect(enc, *protect),
    "dec_srtp_protect": lambda: L.lc3plus_dec_batch_srtp_protect(dec, *protect),
    "srtp_unprotect": lambda: L.lc3plus_dec_batch_srtp_unprotect(dec, 1, A, 64, A, A, 1, A, A, A, A, 10, A, A, A, A, D, L.lc3plus_srtp_workspace_bytes(1, 1), None, 1),
}
assert L.lc3plus_rtcp_workspace_bytes(1, 1) <= 512 and L.lc3plus_srtp_workspace_bytes(1, 1) <= 512
for on in (0, 1, 1):                                                  # off: the device is refused, in front of the library; on, twice: the library is
    L.lc3stub_device_args(on)
    sys.stderr.flush()
    print("round", on, flush=True)
    sys.stderr.write("round %%d\n" %% on)
    for name in %(calls)r:
        print(name, calls[name](), flush=True)
assert not any(a) and not any(d)
L.lc3plus_enc_batch_destroy(enc); L.lc3plus_dec_batch_destroy(dec)
print("done")
"""


def test_a_missing_sibling_fails_its_calls_alone_and_is_named_once():
    subprocess.check_call(["make", "-s", "-C", CSRC, "stub"])
    assert not [f for f in os.listdir(STUB_DIR) if f in SIBLINGS]
    env = dict(os.environ, LC3PLUS_HIP_LIB=os.path.join(STUB_DIR, "liblc3plus_stub.so"))
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, calls=CALLS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, universal_newlines=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = r.stdout.split()
    assert out[-1] == "done"
    results = list(zip(out[:-1:2], out[1:-1:2]))
    assert results == sum(([("round", str(on))] + [(n, str(LC3_ERROR)) for n in CALLS] for on in (0, 1, 1)), [])
    err = r.stderr.splitlines()
    first = err.index("round 1")
    assert err[:first] == ["round 0"]                                   # a call the device refuses does not look for its library
    for f in SIBLINGS:
        assert len([ln for ln in err if f in ln]) == 1, (f, r.stderr)   # the first failure says so; the calls after it, and the second round, are silent
    assert err[-1] == "round 1"                                         # nothing in the second round
