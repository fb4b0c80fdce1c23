"""Secure RTP on the GPU (lc3plus_enc_batch_srtp_protect, lc3plus_dec_batch_srtp_protect, lc3plus_dec_batch_srtp_unprotect; the kernels of
liblc3plus_srtp_hip.so).  Every comparison is equality: the kernels against the host plans (api.plan_srtp_protect, api.plan_srtp_unprotect, themselves held to the
plain Python of srtp_ref.py in test_srtp_cpu.py) on every output array and on the whole destination buffer or ring, guard bytes around every buffer and behind
every array, on the lists of srtp_cases.py: payloads of 0 ... 400 bytes, authenticated lengths on both sides of the SHA-1 padding boundary, all four byte
alignments of source and destination, CSRCs and a header extension, both tag lengths, SEQ crossing 65535, the window's edges, sources that have not started,
flipped bits, 65 items of one source and one item each of 65 sources.  The SSRC table is searched where it lies, not staged in LDS, so no table size takes
another path.  The protect list has its own payloads for the padding boundary (its payload_room shifts it) and slots that hold its 400-byte payloads.  Then both
chains on one HIP stream without a wait between the calls, the host convenience, and the sibling library's own launch counts.  Device buffers through ctypes
(test_gpu_dec_varsize_device._Hip)."""
import numpy as np
import pytest

import srtp_cases as cases
import srtp_gpu_common as common
import srtp_ref as ref
from lc3_harness import sibling_launches
from srtp_gpu_common import SENTINEL, _amd, _dec, _same, _u32, dev   # noqa: F401 (dev: the fixture)

pytestmark = pytest.mark.gpu
KERNELS = ["lc3_srtp_protect_kernel", "lc3_srtp_route_kernel", "lc3_srtp_init_kernel", "lc3_srtp_scan_kernel", "lc3_srtp_auth_kernel", "lc3_srtp_window_kernel",
           "lc3_srtp_state_kernel"]


def _launches(name):
    return sibling_launches("srtp", name)


def _unprotect(dev, bat, c, **kw):
    """the case on the device -> the dict api.plan_srtp_unprotect gives"""
    return common.unprotect(dev, bat, "srtp", c["tag_len"], c, **kw)


def _protect(dev, bat, c, dst_shift, **kw):
    return common.protect(dev, bat, "srtp", c["tag_len"], c, cases.GUARD, dst_shift, **kw)


# ---- unprotect ----
@pytest.mark.parametrize("tag_len", [10, 4])
@pytest.mark.parametrize("which", sorted(cases.CASES))
def test_unprotect_equals_the_host_plan(dev, which, tag_len):
    """every output, the state and the whole ring against lc3plus_plan_srtp_unprotect, and the statuses the scenario is about against what it states.  The
    ring lies at an odd address for one tag length and at an aligned one for the other, so that with the lists' own alignments every datagram alignment occurs
    under both; state_out is state_in for one of them"""
    api = _amd().api
    c = cases.CASES[which](tag_len)
    want = api.plan_srtp_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], tag_len)
    for i, st in c["expect"].items():
        assert want["status"][i] == st, (which, i, int(want["status"][i]), st)
    bat = _dec()
    got = _unprotect(dev, bat, c, in_place=tag_len == 4, ring_shift=1 if tag_len == 10 else 0)
    _same(got, want, which)
    refused = want["status"] != ref.OK
    assert (got["sizes"][refused] == 0).all() and (got["index"][refused] == 0).all()
    bat.close()


def test_unprotect_without_the_optional_outputs(dev):
    api = _amd().api
    c = cases.window(10)
    want = api.plan_srtp_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], 10, optional=())
    bat = _dec()
    _same(_unprotect(dev, bat, c, optional=(), ring_shift=3), want, "no optional outputs")
    bat.close()


def test_split_calls_carry_the_state(dev):
    """one call over the list equals two calls over its halves with the state carried over, on the device as on the host (srtp_cases.split_lists says which
    lists)"""
    c, cut = cases.split_lists(10)
    bat = _dec()
    whole = _unprotect(dev, bat, c)
    a = dict(c, offs=c["offs"][:cut], sizes=c["sizes"][:cut])
    first = _unprotect(dev, bat, a)
    b = dict(c, ring=first["ring"], offs=c["offs"][cut:], sizes=c["sizes"][cut:], state=first["state"])
    second = _unprotect(dev, bat, b)
    assert np.array_equal(whole["state"], second["state"]) and np.array_equal(whole["ring"], second["ring"])
    assert np.array_equal(whole["status"], np.concatenate([first["status"], second["status"]])) and (whole["status"] == ref.OK).all()
    assert np.array_equal(whole["index"], np.concatenate([first["index"], second["index"]]))
    bat.close()


# ---- protect ----
@pytest.mark.parametrize("kind", ["enc", "dec"])
@pytest.mark.parametrize("tag_len", [10, 4])
def test_protect_equals_the_host_plan(dev, tag_len, kind):
    """every output and the whole destination against lc3plus_plan_srtp_protect, the plan's statuses against what the list was built for, and the packets'
    rollover counters against the list's own count across 65535 -> 0.  The arrays behind n_packets keep their sentinel"""
    api = _amd().api
    c = cases.protect_list(tag_len)
    m, k = c["max_packets"], c["n_packets"]
    dst0 = np.full(c["dst_capacity"], 0x6B, np.uint8)
    want = api.plan_srtp_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], dst0, c["stride"], tag_len, c["hr"], c["pr"],
                                 next_seq=c["next_seq"], n_packets=k)
    for i, st in c["expect"].items():
        assert want["out_status"][i] == st, (i, int(want["out_status"][i]), st)
    assert np.array_equal(want["next_roc"], _u32([0, 6]))             # route 0 crossed 65535 from ROC FFFFFFFF: 0; route 1 did not
    bat = _amd().Batch(2, 48000, 1, 10.0, 0, [64000] * 2, device=0) if kind == "enc" else _dec(2)
    got = _protect(dev, bat, c, dst_shift=2 if tag_len == 10 else 0, with_next=kind == "enc")
    for name in ("out_offset", "out_size", "out_status"):
        assert np.array_equal(got[name][:k], want[name][:k]), name
        assert (got[name][k:] == SENTINEL[got[name].dtype.type]).all(), (name, "written behind n_packets")
    bad = np.argwhere(got["dst"] != want["dst"])
    assert len(bad) == 0, ("dst: first differing bytes", bad[:6].ravel().tolist())
    if kind == "enc":
        assert np.array_equal(got["next_roc"], want["next_roc"])
    bat.close()


# ---- the chains ----
@pytest.mark.parametrize("tag_len", [10, 4])
def test_sender_to_receiver_without_a_host_wait(dev, tag_len):
    """encode_packed -> egress -> stamp -> protect and unprotect -> parse -> probe -> ingest on the protect call's output, all queued on one HIP stream with
    sync = 0 and one wait at the end.  The protected packets are the host plan's on the stamped wire buffer; every frame the egress sent stands in the ingest's
    tables, byte for byte the oracle encoder's, and the receiver's state has advanced to every route's last sequence number across 65535 -> 0"""
    common.sender_to_receiver(dev, "srtp", tag_len, cases, ref)


def test_host_convenience_equals_the_host_plan():
    """DecBatch.srtp_unprotect - upload, run, download - gives the dict api.plan_srtp_unprotect gives, with and without the optional outputs"""
    api = _amd().api
    bat = _dec()
    for which, tag_len, optional in (("tampered", 10, api.SRTP_UNPROTECT_OPTIONAL), ("rollover", 4, ("index",))):
        c = cases.CASES[which](tag_len)
        got = bat.srtp_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], tag_len, optional=optional)
        want = api.plan_srtp_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], tag_len, optional=optional)
        assert set(got) == set(want)
        _same(got, want, which)
    bat.close()


def test_every_srtp_kernel_ran_under_a_comparison(dev):
    """a protect call with next_roc launches the protect and the route kernel once each, an unprotect call its five kernels once each"""
    api = _amd().api
    before = {k: _launches(k) for k in KERNELS}
    assert all(v >= 0 for v in before.values()) and _launches("no_such_kernel") == -1
    bat = _dec(2)
    c = cases.protect_list(10)
    got = _protect(dev, bat, c, dst_shift=1)
    want = api.plan_srtp_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"], np.full(c["dst_capacity"], 0x6B, np.uint8),
                                 c["stride"], 10, c["hr"], c["pr"], next_seq=c["next_seq"], n_packets=c["n_packets"])
    assert np.array_equal(got["dst"], want["dst"])
    u = cases.fresh(10)
    _same(_unprotect(dev, bat, u), api.plan_srtp_unprotect(u["ring"], u["offs"], u["sizes"], u["ssrc_key"], u["ctx"], u["state"], 10), "fresh")
    for k in KERNELS:
        assert _launches(k) == before[k] + 1, k
    bat.close()
