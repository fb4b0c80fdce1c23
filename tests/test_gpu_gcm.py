"""Secure RTP with AES-GCM on the GPU (lc3plus_enc_batch_srtp_gcm_protect, lc3plus_dec_batch_srtp_gcm_protect, lc3plus_dec_batch_srtp_gcm_unprotect; the
kernels of liblc3plus_gcm_hip.so).  Every comparison is equality: the kernels against the host plans (api.plan_srtp_gcm_protect, api.plan_srtp_gcm_unprotect,
themselves held to the plain Python of gcm_ref.py and through it to libcrypto in test_gcm_cpu.py) on every output array and on the whole destination buffer or
ring, guard bytes around every buffer and behind every array, on the lists of gcm_cases.py: payloads of 0 ... 400 bytes around one, two and three AES blocks,
headers of 12 to 28 and 80 bytes, all four byte alignments of source and destination, 16- and 32-byte keys side by side in every call, SEQ crossing 65535, the
window's edges, sources that have not started, flipped bits, and lists of more than one workgroup.  The kernels read keys, round counts and GHASH tables where
the contexts lie, so no table size takes another path.  Then both chains on one HIP stream without a wait between the calls, the host convenience, and the
sibling library's own launch counts.  Device buffers through ctypes (test_gpu_dec_varsize_device._Hip)."""
import numpy as np
import pytest

import gcm_cases as cases
import gcm_ref as ref
import srtp_gpu_common as common
from lc3_harness import sibling_launches
from srtp_gpu_common import SENTINEL, _amd, _dec, _same, _u32, dev   # noqa: F401 (dev: the fixture)

pytestmark = pytest.mark.gpu
KERNELS = ["lc3_gcm_protect_kernel", "lc3_gcm_route_kernel", "lc3_gcm_init_kernel", "lc3_gcm_scan_kernel", "lc3_gcm_auth_kernel", "lc3_gcm_window_kernel",
           "lc3_gcm_state_kernel"]


def _launches(name):
    return sibling_launches("gcm", name)


def _plan_unprotect(c, **kw):
    return _amd().api.plan_srtp_gcm_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], **kw)


# ---- unprotect ----
def _unprotect(dev, bat, c, **kw):
    """the case on the device -> the dict api.plan_srtp_gcm_unprotect gives"""
    return common.unprotect(dev, bat, "srtp_gcm", None, c, **kw)


@pytest.mark.parametrize("ring_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("which", sorted(cases.CASES))
def test_unprotect_equals_the_host_plan(dev, which, ring_shift):
    """every output, the state and the whole ring against lc3plus_plan_srtp_gcm_unprotect, and the statuses the scenario is about against what it states, with
    the ring 0 to 3 bytes behind an aligned address; state_out is state_in for the odd shifts"""
    c = cases.CASES[which]()
    want = _plan_unprotect(c)
    for i, st in c["expect"].items():
        assert want["status"][i] == st, (which, i, int(want["status"][i]), st)
    bat = _dec()
    got = _unprotect(dev, bat, c, in_place=ring_shift & 1, ring_shift=ring_shift)
    _same(got, want, which)
    refused = want["status"] != ref.OK
    assert (got["sizes"][refused] == 0).all() and (got["index"][refused] == 0).all()
    bat.close()


def test_unprotect_without_the_optional_outputs(dev):
    c = cases.window()
    want = _plan_unprotect(c, optional=())
    bat = _dec()
    _same(_unprotect(dev, bat, c, optional=(), ring_shift=3), want, "no optional outputs")
    bat.close()


def test_split_calls_carry_the_state(dev):
    """one call over the list equals two calls over its halves with the state carried over, on the device as on the host"""
    c, cut = cases.split_lists()
    bat = _dec()
    whole = _unprotect(dev, bat, c)
    a = dict(c, offs=c["offs"][:cut], sizes=c["sizes"][:cut])
    first = _unprotect(dev, bat, a)
    b = dict(c, ring=first["ring"], offs=c["offs"][cut:], sizes=c["sizes"][cut:], state=first["state"])
    second = _unprotect(dev, bat, b)
    assert np.array_equal(whole["state"], second["state"]) and np.array_equal(whole["ring"], second["ring"])
    assert np.array_equal(whole["status"], np.concatenate([first["status"], second["status"]])) and (whole["status"] == ref.OK).all()
    assert np.array_equal(whole["index"], np.concatenate([first["index"], second["index"]]))
    _same(whole, _plan_unprotect(c), "the whole list")
    bat.close()


# ---- protect ----
def _protect(dev, bat, c, dst_shift, **kw):
    return common.protect(dev, bat, "srtp_gcm", None, c, cases.GUARD, dst_shift, **kw)


def _plan_protect(c):
    return _amd().api.plan_srtp_gcm_protect(c["route"], c["off"], c["size"], c["status"], c["wire"], c["ctx"], c["roc"], c["seq_base"],
                                            np.full(c["dst_capacity"], 0x6B, np.uint8), c["stride"], c["hr"], c["pr"], next_seq=c["next_seq"], n_packets=c["n_packets"])


@pytest.mark.parametrize("kind", ["enc", "dec"])
@pytest.mark.parametrize("dst_shift", [0, 1, 2, 3])
def test_protect_equals_the_host_plan(dev, dst_shift, kind):
    """every output and the whole destination, guards included, against lc3plus_plan_srtp_gcm_protect, the plan's statuses against what the list was built
    for, and the packets' rollover counters against the list's own count across 65535 -> 0.  The arrays behind n_packets keep their sentinel"""
    c = cases.protect_list()
    k = c["n_packets"]
    want = _plan_protect(c)
    for i, st in c["expect"].items():
        assert want["out_status"][i] == st, (i, int(want["out_status"][i]), st)
    assert np.array_equal(want["next_roc"], _u32([0, 6]))             # route 0 crossed 65535 from ROC FFFFFFFF: 0; route 1 did not
    bat = _amd().Batch(2, 48000, 1, 10.0, 0, [64000] * 2, device=0) if kind == "enc" else _dec(2)
    got = _protect(dev, bat, c, dst_shift=dst_shift, with_next=kind == "enc")
    for name in ("out_offset", "out_size", "out_status"):
        assert np.array_equal(got[name][:k], want[name][:k]), name
        assert (got[name][k:] == SENTINEL[got[name].dtype.type]).all(), (name, "written behind n_packets")
    bad = np.argwhere(got["dst"] != want["dst"])
    assert len(bad) == 0, ("dst: first differing bytes", bad[:6].ravel().tolist())
    if kind == "enc":
        assert np.array_equal(got["next_roc"], want["next_roc"])
    bat.close()


# ---- the chains ----
def test_sender_to_receiver_without_a_host_wait(dev):
    """encode_packed -> egress -> stamp -> gcm_protect and gcm_unprotect -> parse -> probe -> ingest on the protect call's output, all queued on one HIP stream
    with sync = 0 and one wait at the end, 6 streams whose routes alternate 16- and 32-byte keys, across a sequence wrap.  The protected packets are the host
    plan's on the stamped wire buffer; every frame the egress sent stands in the ingest's tables, byte for byte the oracle encoder's, and the receiver's state
    has advanced to every route's last sequence number across 65535 -> 0"""
    run = common.sender_to_receiver(dev, "srtp_gcm", None, cases, ref)
    assert run["S"] == 6
    assert run["ctx"][:, 60].tolist() == [10, 14] * 3
    assert run["wrapped"].any()


def test_host_convenience_equals_the_host_plan():
    """DecBatch.srtp_gcm_unprotect - upload, run, download - gives the dict api.plan_srtp_gcm_unprotect gives, with and without the optional outputs"""
    api = _amd().api
    bat = _dec()
    for which, optional in (("tampered", api.SRTP_UNPROTECT_OPTIONAL), ("rollover", ("index",))):
        c = cases.CASES[which]()
        got = bat.srtp_gcm_unprotect(c["ring"], c["offs"], c["sizes"], c["ssrc_key"], c["ctx"], c["state"], optional=optional)
        want = _plan_unprotect(c, optional=optional)
        assert set(got) == set(want)
        _same(got, want, which)
    bat.close()


def test_every_gcm_kernel_ran_under_a_comparison(dev):
    """a protect call with next_roc launches the protect and the route kernel once each, an unprotect call its five kernels once each; no kernel of the SRTP
    library is this library's"""
    before = {k: _launches(k) for k in KERNELS}
    assert all(v >= 0 for v in before.values()) and _launches("no_such_kernel") == -1 and _launches("lc3_srtp_auth_kernel") == -1
    bat = _dec(2)
    c = cases.protect_list()
    got = _protect(dev, bat, c, dst_shift=1)
    assert np.array_equal(got["dst"], _plan_protect(c)["dst"])
    u = cases.fresh()
    _same(_unprotect(dev, bat, u), _plan_unprotect(u), "fresh")
    for k in KERNELS:
        assert _launches(k) == before[k] + 1, k
    bat.close()
