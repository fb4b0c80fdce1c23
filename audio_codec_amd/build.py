"""Builds liblc3plus_hip.so, the frame probe's liblc3plus_probe_hip.so, the packet ingest's liblc3plus_ingest_hip.so, the packet egress's
liblc3plus_egress_hip.so, the RTP framing's liblc3plus_rtp_hip.so, the reception reports' liblc3plus_rtcp_hip.so and Secure RTP's liblc3plus_srtp_hip.so in-tree
(hipcc cross-compiles gfx950 without a GPU)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def build(verbose=False):
    cmd = ["make", "-j%d" % max(1, min(16, os.cpu_count() or 1)), "-C", os.path.join(HERE, "csrc")]   # the kernel objects, the runtime, the probe, the ingest, the egress, the RTP, the reception report and the SRTP library, independent of each other
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return os.path.join(HERE, "liblc3plus_hip.so")
