"""Reception reports without a GPU (include/lc3plus_batch.h "Reception reports"): the exported symbols and constants, every refusal of the batch call in the
header's order (its checks run before anything of the batch or the device is touched), lc3plus_plan_rtcp_stats - the text the kernels run - against the plain
Python restatement of the rule (rtcp_ref.stats) on every output, the split property at every cut, the blocks against what the ingest says of the same items, and
the host code once more in a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tools/rtcp_plan_driver.c).  Every comparison is
equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api, packet
import rtcp_ref as ref

NEW = ["lc3plus_dec_batch_rtcp_stats", "lc3plus_plan_rtcp_stats", "lc3plus_rtcp_workspace_bytes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_codec_amd", "csrc")
LC3_OK, LC3_ERROR, LC3_NULL_ERROR = 0, 1, 3
ARGS = ("n_items", "stream", "seq", "timestamp", "arrival", "n_streams", "state_in", "state_out", "make_report", "ssrc", "lsr", "dlsr", "blocks", "ext_seq",
        "item_status", "stream_stats")
TAIL = ("workspace", "workspace_bytes", "hip_stream", "sync")
REQUIRED = ("stream", "seq", "timestamp", "arrival", "state_in", "state_out")
NULLABLE = ("lsr", "dlsr", "ext_seq", "item_status", "stream_stats")
VALUES = dict(n_items=1, n_streams=1, make_report=1, workspace_bytes=1 << 20, hip_stream=None, sync=1)
BAD = (dict(n_items=0), dict(n_items=-1), dict(n_items=1 << 29), dict(n_items=(1 << 63) - 1), dict(n_streams=0), dict(n_streams=-2), dict(make_report=2),
       dict(make_report=-1), dict(make_report=256))
SETS = ref.cpu_sets()


def test_symbols_are_exported():
    L = audio_codec_amd.load_library()
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    for s in NEW:
        assert s in api.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, text), s
    assert callable(api.DecBatch.rtcp_stats_device) and callable(api.DecBatch.rtcp_stats) and callable(api.plan_rtcp_stats) and callable(api.rtcp_workspace_bytes)
    assert os.path.exists(os.path.join(ROOT, "audio_codec_amd", "liblc3plus_rtcp_hip.so"))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lc3plus_batch.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+LC3PLUS_RR_(\w+)\s+(\d+)", text)}
    want = dict(FLAGS=0, BASE_SEQ=1, MAX_SEQ=2, CYCLES=3, BAD_SEQ=4, RECEIVED=5, EXPECTED_PRIOR=6, RECEIVED_PRIOR=7, TRANSIT=8, JITTER=9, STATE_WORDS=10, STARTED=1,
                DROPPED=0, COUNTED=1, JUMP=2, RESTART=3, REORDERED=4, ST_COUNTED=0, ST_JUMP=1, ST_RESTART=2, ST_REORDERED=3, STATS_WORDS=4, BLOCK_BYTES=24,
                MAX_DROPOUT=3000, MAX_MISORDER=100)
    assert header == want
    for k, v in want.items():
        assert getattr(api, "RR_" + k) == v == getattr(ref, k), k
    assert api.RR_OUTPUTS == ref.KEYS


def test_workspace_bytes():
    assert api.rtcp_workspace_bytes(0, 1) == api.rtcp_workspace_bytes(1, 0) == api.rtcp_workspace_bytes(1 << 29, 1) == api.rtcp_workspace_bytes(-1, 1) == 0
    # the scratch of the four steps: two words per stream, one per item, and a little more
    for n, S in ((1, 1), (262144, 4096), ((1 << 29) - 1, 1), (5, 1 << 20)):
        w = api.rtcp_workspace_bytes(n, S)
        assert 4 * (n + 2 * S) <= w <= 4 * (n + 3 * S) + 64, (n, S, w)


def test_refusals_need_no_device():
    """a zero-filled block stands in for the batch: no refusal writes to it or to an array"""
    L = audio_codec_amd.load_library()
    fake, arr = C.create_string_buffer(4096), C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS + TAIL}, b=C.cast(fake, C.c_void_p), **VALUES)

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_dec_batch_rtcp_stats(a["b"], *[a[k] for k in ARGS + TAIL])
    assert call(b=None) == LC3_NULL_ERROR and call(b=None, n_items=0) == LC3_NULL_ERROR and call(b=None, stream=None, make_report=5) == LC3_NULL_ERROR
    for k in REQUIRED + ("workspace", "ssrc", "blocks"):
        assert call(**{k: None}) == LC3_NULL_ERROR, k
        for kw in (BAD[0], BAD[4], dict(workspace_bytes=0)):                           # NULL first
            assert call(**dict(kw, **{k: None})) == LC3_NULL_ERROR, (k, kw)
    for k in NULLABLE:
        for kw in BAD[:2]:
            assert call(**dict(kw, **{k: None})) == LC3_ERROR, (k, kw)                # an optional NULL is no refusal: the value check behind it answers
    for kw in BAD:
        assert call(**kw) == LC3_ERROR, kw
    assert call(make_report=0, ssrc=None, blocks=None, n_items=0) == LC3_ERROR         # without make_report neither is needed
    need = api.rtcp_workspace_bytes(1, 1)
    assert call(workspace_bytes=need - 1) == LC3_ERROR and call(workspace_bytes=0) == LC3_ERROR and call(workspace_bytes=-1) == LC3_ERROR
    need = api.rtcp_workspace_bytes(1000, 70)
    assert call(n_items=1000, n_streams=70, workspace_bytes=need - 1) == LC3_ERROR
    assert fake.raw == bytes(4096) and arr.raw == bytes(256)


def test_plan_refusals():
    L = audio_codec_amd.load_library()
    arr = C.create_string_buffer(256)
    p = C.cast(arr, C.c_void_p)
    good = dict({k: p for k in ARGS}, **{k: v for k, v in VALUES.items() if k in ARGS})

    def call(**kw):
        a = dict(good, **kw)
        return L.lc3plus_plan_rtcp_stats(*[a[k] for k in ARGS])
    for k in REQUIRED + ("ssrc", "blocks"):
        assert call(**{k: None}) == LC3_NULL_ERROR and call(**dict(BAD[0], **{k: None})) == LC3_NULL_ERROR, k
    for kw in BAD:
        assert call(**kw) == LC3_ERROR, kw
    assert arr.raw == bytes(256)
    assert call(make_report=0, ssrc=None, blocks=None, lsr=None, dlsr=None, ext_seq=None, item_status=None, stream_stats=None) == LC3_OK
    with pytest.raises(api.LC3Error):
        api.plan_rtcp_stats([], [], [], [], np.zeros((1, 10)))


def plan(c, make_report=True, optional=api.RR_OPTIONAL, state=None):
    return api.plan_rtcp_stats(c["stream"], c["seq"], c["timestamp"], c["arrival"], c["state"] if state is None else state, make_report, c["ssrc"], c["lsr"], c["dlsr"],
                               optional)


def same(got, want, name, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (name, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", list(SETS))
def test_plan_equals_the_rule(name):
    """every output, with and without make_report, with lsr and dlsr NULL and with each optional output alone"""
    c = SETS[name]
    for make_report in (True, False):
        want = ref.stats(c, make_report)
        same(plan(c, make_report), want, (name, make_report))
    bare = dict(c, lsr=None, dlsr=None)
    same(plan(bare), ref.stats(bare), (name, "no lsr"))
    want = ref.stats(c)
    for optional in ((),) + tuple((k,) for k in api.RR_OPTIONAL):
        got = plan(c, True, optional)
        assert all(got[k] is None for k in api.RR_OPTIONAL if k not in optional)
        same(got, want, (name, optional), ("state", "blocks") + optional)


def test_the_rule_by_hand():
    """the restatement itself against values worked out by hand from the header's text"""
    c, at = ref.patterns()
    r = ref.stats(c)
    st = lambda nm: r["item_status"][c["stream"] == at[nm]].tolist()
    ext = lambda nm: r["ext_seq"][c["stream"] == at[nm]].tolist()
    blk = lambda nm: ref.block_fields(r["blocks"][at[nm]])
    assert st("one") == [1] and ext("one") == [7] and blk("one")["lost"] == 0 and blk("one")["ext_high"] == 7
    assert st("wrap") == [1, 1, 1, 1] and ext("wrap") == [65534, 65535, 65536, 65537] and blk("wrap")["ext_high"] == 65537 and blk("wrap")["lost"] == 0
    assert st("reordered_across_wrap") == [1, 1, 4, 1] and ext("reordered_across_wrap") == [65534, 65536, 65535, 65537]
    assert st("duplicate") == [1, 1, 1, 1] and ext("duplicate") == [10, 11, 11, 12] and blk("duplicate")["lost"] == -1    # udelta 0 is in order: counted twice
    assert st("dropout_2999") == [1, 1, 1] and blk("dropout_2999")["lost"] == 2998 and blk("dropout_2999")["fraction"] == (2998 << 8) // 3001
    assert st("dropout_3000") == [1, 2, 1] and ext("dropout_3000") == [100, 0, 101]
    assert st("misorder_65436") == [1, 2, 1] and st("misorder_65437") == [1, 4, 1] and ext("misorder_65437") == [100, 1, 101]
    assert st("misorder_wrapped") == [1, 2, 4]                        # 100 back is a jump, 99 back is reordered
    assert st("jump_then_successor") == [1, 2, 3, 1] and ext("jump_then_successor") == [100, 0, 5001, 5002]
    assert r["state"][at["jump_then_successor"]][[ref.BASE_SEQ, ref.MAX_SEQ, ref.RECEIVED]].tolist() == [5001, 5002, 2]
    assert st("jump_then_other") == [1, 2, 2, 1, 3, 1] and r["stream_stats"][at["jump_then_other"]].tolist() == [4, 2, 1, 0]
    assert st("jump_then_same") == [1, 2, 2, 1] and st("restart_at_wrap") == [1, 2, 3, 1] and ext("restart_at_wrap") == [100, 0, 0, 1]
    assert st("seq_above_16_bits") == [1, 1, 1] and ext("seq_above_16_bits") == [5, 6, 7]
    c, at = ref.crafted_states()
    r = ref.stats(c)
    f = lambda nm: ref.block_fields(r["blocks"][at[nm]])
    assert f("lost_below")["lost"] == -0x800000 and f("lost_above")["lost"] == 0x7FFFFF and f("lost_edges")["lost"] == 0x7FFFFF
    assert f("fraction_cap")["fraction"] == 255 and f("fraction_half")["fraction"] == 128 and f("negative_interval")["fraction"] == 0x40
    assert f("jump_only")["fraction"] == 0 and f("jump_only")["jitter"] == 0x12 and r["item_status"].tolist() == [ref.JUMP, ref.COUNTED, ref.DROPPED]
    assert r["state"][at["jump_only"]][ref.BAD_SEQ] == 40001
    assert not r["blocks"][at["not_started"]].any() and not r["state"][at["not_started"]].any()
    assert r["state"][at["flag_bits"]][ref.FLAGS] == 0x7FFFFFF1 and r["state"][at["not_started_bits"]].tolist() == [7, 9, 9, 0, 65537, 1, 1, 1, 77, 0]
    w = [0] * 10                                                     # stream 1 of transits, step by step: d = 0x80000000 counts as 2^31 whichever way it points
    assert ref.item(w, 1, 0, 0) == (1, 1) and ref.item(w, 2, 0, 0x80000000) == (1, 2) and w[ref.JITTER] == 0x80000000
    j = 0x80000000
    assert ref.item(w, 3, 0, 0)[0] == 1 and w[ref.JITTER] == (j + 0x80000000 - ((j + 8) >> 4)) & ref.M


@pytest.mark.parametrize("name", ["patterns", "transits", "traffic_5x40", "one_stream_129", "crafted_states"])
def test_split_at_every_position(name):
    """a set cut in two at every position, the state carried, a report only in the second call, equals one call"""
    c = SETS[name]
    whole = plan(c)
    n = len(c["stream"])
    for k in range(1, n):
        a, b = ref.split(c, k)
        first = plan(a, False)
        second = plan(b, True, state=first["state"])
        assert first["blocks"] is None
        assert np.array_equal(second["state"], whole["state"]) and np.array_equal(second["blocks"], whole["blocks"]), k
        assert np.array_equal(np.concatenate([first["ext_seq"], second["ext_seq"]]), whole["ext_seq"]), k
        assert np.array_equal(np.concatenate([first["item_status"], second["item_status"]]), whole["item_status"]), k
        assert np.array_equal(first["stream_stats"] + second["stream_stats"], whole["stream_stats"]), k


def test_in_place_state():
    """state_in and state_out as one array"""
    L = audio_codec_amd.load_library()
    c = SETS["traffic_5x40"]
    want = plan(c)
    a = packet._rtcp_arrays(c["stream"], c["seq"], c["timestamp"], c["arrival"], c["state"], True, c["ssrc"], c["lsr"], c["dlsr"], ())
    state = a["state_in"].copy()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = L.lc3plus_plan_rtcp_stats(a["stream"].size, ptr(a["stream"]), ptr(a["seq"]), ptr(a["timestamp"]), ptr(a["arrival"]), state.shape[0], ptr(state), ptr(state), 1,
                                   ptr(a["ssrc"]), ptr(a["lsr"]), ptr(a["dlsr"]), ptr(a["blocks"]), None, None, None)
    assert rc == 0 and np.array_equal(state, want["state"]) and np.array_equal(a["blocks"], want["blocks"])


@pytest.mark.parametrize("seed,S,T", [(11, 6, 50), (12, 40, 20), (13, 3, 300)])
def test_blocks_agree_with_the_ingest(seed, S, T):
    """lossy, reordered traffic without duplicates or restarts, every stream's first packet first: the block's cumulative loss is the ingest's gap count and its
    extended highest sequence number the ingest's next_base - 1, extended by the cycles"""
    c = ref.traffic(seed, S, T, bad_items=0.05, with_faults=False)
    r = plan(c)
    assert set(r["item_status"].tolist()) == {api.RR_DROPPED, api.RR_COUNTED}
    base = r["state"][:, api.RR_BASE_SEQ]
    n = len(c["stream"])
    ing = api.plan_ingest(S, 1, c["stream"], c["seq"], np.arange(n), np.ones(n), base, T, 16)
    assert ing["stats"][:, 1].sum() > 0 and (base + T > 65536).any()
    for s in range(S):
        f = ref.block_fields(r["blocks"][s])
        assert f["lost"] == ing["stats"][s, 1], s
        assert f["ext_high"] == int(base[s]) + int(ing["counts"][s]) - 1 and f["ext_high"] & 0xFFFF == (int(ing["next_base"][s]) - 1) & 0xFFFF, s
        assert f["ssrc"] == int(c["ssrc"][s]) and f["lsr"] == int(c["lsr"][s]) and f["dlsr"] == int(c["dlsr"][s])


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, "rtcp_driver"])
    return os.path.join(ROOT, "audio_codec_amd", "_stub", "rtcp_plan_driver")


class _Lcg:
    def __init__(self, seed):
        self.x = seed

    def __call__(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7FFFFFFF
        return self.x >> 8


def _driver_case(seed, N, S):
    """the case tools/rtcp_plan_driver.c draws from these arguments"""
    lcg, M = _Lcg(seed), ref.M
    nxt, ssrc, lsr, dlsr, state = [], [], [], [], []
    for k in range(S):
        nxt.append(65530 if lcg() & 1 else lcg() & 0xFFFF)
        ssrc.append((0x80000001 + k * 0x3FFFFFFF) & M)
        lsr.append(lcg() * 2654435761 & M)
        dlsr.append(lcg())
        w = [0] * 10
        if k % 3 == 1:
            w[0], w[1], w[2] = 1, lcg() & 0xFFFF, (nxt[k] - 1) & 0xFFFF
            w[3] = ((lcg() & 0xFF) << 16) * (0x101 if k % 2 else 1) & M
            w[4], w[5], w[6], w[7], w[8] = 65537, lcg() * 517 & M, lcg() * 3 & M, lcg() * 5 & M, lcg() * 2654435761 & M
            w[9] = lcg() & 0xFFFFF
        state.append(w)
    stream, seq, ts, arr = [], [], [], []
    for _ in range(N):
        d = lcg()
        k = -1 if d % 23 == 0 else S if d % 29 == 0 else (d >> 4) % S
        stream.append(k)
        q = lcg()
        if 0 <= k < S:
            e = lcg() % 40
            if e == 0:
                nxt[k] = (nxt[k] + 3000 + lcg() % 60000) & M
            elif e == 1:
                nxt[k] = (nxt[k] - 1 - lcg() % 3) & M
            elif e == 2:
                nxt[k] = (nxt[k] + 1 + lcg() % 5) & M
            q = (nxt[k] + ((lcg() & 1) << 16)) & M
            nxt[k] = (nxt[k] + 1) & M
        seq.append(q)
        ts.append((q * 480 + 0xFFFF0000) & M)
        far = 0x80000000 if lcg() % 7 == 0 else 0
        arr.append((ts[-1] + far + lcg() % 1000) & M)
    c = ref.case(stream, seq, ts, arr, S, state)
    return dict(c, ssrc=np.array(ssrc, np.int64), lsr=np.array(lsr, np.int64), dlsr=np.array(dlsr, np.int64))


@pytest.mark.parametrize("argv", [(1, 500, 7, 1, 0), (2, 2000, 40, 1, 1), (3, 1, 1, 1, 0), (4, 300, 2, 0, 1), (5, 64, 100, 1, 0)])
def test_plan_under_sanitizers(driver, argv):
    """lc3plus_plan_rtcp_stats in a program of its own under ASan + UBSan, every array a heap block of its exact size: a clean exit, and its output is the rule's"""
    p = subprocess.run([driver, "stats"] + [str(a) for a in argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines()}
    assert out["rc"] == [0]
    seed, N, S, report, _ = argv
    c = _driver_case(seed, N, S)
    want = ref.stats(c, bool(report))
    for k in ref.KEYS:
        if want[k] is None:
            assert set(out[k]) == {0x5A}, k                           # blocks is not written without make_report
        else:
            assert out[k] == want[k].reshape(-1).tolist(), k
    assert out["workspace"] == [api.rtcp_workspace_bytes(N, S)]
    assert N < 100 or len(set(want["item_status"].tolist())) == 5


def test_refusals_under_sanitizers(driver):
    p = subprocess.run([driver, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("refusals ok"), (p.stdout[-400:], p.stderr[-2000:])
