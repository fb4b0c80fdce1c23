"""Packet ingest on the GPU (lc3plus_dec_batch_ingest; the four kernels of liblc3plus_ingest_hip.so).  Every output array is held to equality: the kernels against
the host plan (api.plan_ingest, itself held to the numpy rule in test_ingest_cpu.py) on lists that fill neither waves nor workgroups evenly, with guard words
behind every output; then probe -> ingest -> set_frame_counts + decode_packed queued on one HIP stream with a single wait at the end, PCM and status against
the CPU oracle decoder run over the sequence each stream is expected to see; statelessness; and the sibling library's own launch counts.  Device buffers through
ctypes (test_gpu_dec_varsize_device._Hip)."""
import functools
import os
import sys

import numpy as np
import pytest

import hostile_frames as hf
import ingest_ref as ref
from lc3_harness import sibling_launches
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # elements behind every output array
E2E_GEOMS = ("48k_10_128B", "48k_10_stereo_161B")      # one mono, one stereo geometry of frame_probe_ref
KERNELS = ["lc3_ingest_fill_kernel", "lc3_ingest_item_kernel", "lc3_ingest_status_kernel", "lc3_ingest_stream_kernel"]


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


def _sentinel(dtype):
    return {np.int64: 0x5A5A5A5A5A5A5A5A, np.int32: 0x5A5A5A5A, np.uint8: 0x5A}[dtype]


def _run(dev, d, c, optional=None, hip_stream=None):
    """one ingest call with sync on batch d -> dict as api.plan_ingest gives; every output lies in front of GUARD sentinel elements, which must come back
    untouched, and holds the sentinel itself beforehand"""
    api = _amd().api
    optional = api.ING_OPTIONAL if optional is None else optional
    S, T, n = c["n_streams"], c["n_frames"], len(c["stream"])
    shapes = dict(offsets=((S, T), np.int64), num_bytes=((S, T), np.int32), cell_item=((S, T), np.int32), counts=((S,), np.int32), next_base=((S,), np.int32),
                  stats=((S, api.ING_STATS_WORDS), np.int32), item_status=((n,), np.uint8))
    ptr = {}
    for k, (shape, dt) in shapes.items():
        ptr[k] = dev.put(np.full(int(np.prod(shape)) + GUARD, _sentinel(dt), dt)) if k in ref.KEYS[:4] or k in optional else None
    d.ingest_device(n, dev.put(c["stream"]), dev.put(c["seq"]), dev.put(c["offsets"]), dev.put(c["num_bytes"]), dev.put(c["base"]), T, ptr["offsets"],
                    ptr["num_bytes"], ptr["cell_item"], ptr["counts"], c["seq_bits"], dev.put(c["info"]) if c["info"] is not None else None,
                    dev.put(c["floor"]) if c["floor"] is not None else None, ptr["next_base"], ptr["stats"], ptr["item_status"], hip_stream, sync=True)
    out = {}
    for k, (shape, dt) in shapes.items():
        if ptr[k] is None:
            out[k] = None
            continue
        size = int(np.prod(shape))
        got = dev.get(ptr[k], (size + GUARD,), dt)
        assert (got[size:] == _sentinel(dt)).all(), ("a word behind the output was written", k)
        out[k] = got[:size].reshape(shape)
    return out


def _plan(c, optional=None):
    api = _amd().api
    return api.plan_ingest(c["n_streams"], c["channels"], c["stream"], c["seq"], c["offsets"], c["num_bytes"], c["base"], c["n_frames"], c["seq_bits"], c["info"],
                           c["floor"], api.ING_OPTIONAL if optional is None else optional)


def _same(got, want, name, keys=ref.KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (name, k, "first differences at", bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def _batch(S, ch):
    return _amd().DecBatch(S, 48000, ch, 10.0, 0, None, device=0)


@pytest.mark.parametrize("name", list(ref.gpu_lists()))
def test_kernels_equal_the_host_plan(dev, name):
    """every output array of the four kernels against lc3plus_plan_ingest and against the numpy rule; once more with every optional output NULL (no status
    kernel, no counting), on a second HIP stream"""
    c = ref.gpu_lists()[name]
    want = _plan(c)
    _same(want, ref.rule(c), (name, "plan against the rule"))
    d = _batch(c["n_streams"], c["channels"])
    _same(_run(dev, d, c), want, name)
    got = _run(dev, d, c, optional=(), hip_stream=dev.stream())
    assert got["next_base"] is None and got["stats"] is None and got["item_status"] is None
    _same(got, want, (name, "optional outputs NULL"), ref.KEYS[:4])
    d.close()


@functools.lru_cache(maxsize=None)
def _scenario(geom):
    """A receive buffer for four streams of hostile_frames.streams(geom) x 24 frames.  Where the stream's own frame is genuine or accepted it is the cell's good
    copy: most cells get it alone, some get a refused copy in front of it (earlier in the list), some get the refused copy alone, some nothing; where the
    stream's own frame is refused, it is the cell's only copy.  The last stream's last five frames have not arrived; stream 0 misses its last frame but has a
    floor of 24.  Beside them one item each that is late, early, empty, for a stream that does not exist, a second copy of a frame and an invalid one.
    -> dict: buf, items (stream, seq, offsets, num_bytes), base, floor, and what each stream is expected to decode: frames [B, T, stride], sizes [B, T],
    counts [B]"""
    fs, ms, hr, ch, zs = hf.GEOMS[geom]
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    pats = hf.patterns(geom)
    rows = [pats.index(p) for p in ("r_behind_g", "r_first", "alternating", "all_h")]
    B, T = len(rows), hf.T
    size = int(sizes[rows[0], 0])
    assert (sizes[rows] == size).all() and np.isin(kind[rows], (hf.G, hf.H, hf.R)).all()
    refused = [frames[b, t, :size] for b in rows for t in range(T) if kind[b, t] == hf.R]
    rng = np.random.RandomState(len(geom) * 101)
    base = np.array([65530, 65535, 7, 65536 - T + 1])            # three of the four streams pass 65535 inside the call
    exp_frames, exp_sizes = np.zeros((B, T, frames.shape[2]), np.uint8), np.zeros((B, T), np.int32)
    items, must_precede, census = [], [], dict(both=0, good=0, corrupt=0, missing=0)      # item: (stream, seq, payload)
    for s, b in enumerate(rows):
        for t in range(T):
            own, bad = frames[b, t, :size], refused[rng.randint(len(refused))]
            r = rng.randint(0, 10)
            if (s == B - 1 and t >= T - 5) or (s == 0 and t == T - 1):
                what = "missing"
            elif kind[b, t] == hf.R:
                what, bad = "corrupt", own
            elif t == 0:
                what = "good"
            else:
                what = "both" if r < 3 else "missing" if r == 3 else "corrupt" if r == 4 else "good"
            census[what] += 1
            seq = (base[s] + t) & 0xFFFF
            if what in ("both", "corrupt"):
                items.append((s, seq, bad))
            if what in ("both", "good"):
                items.append((s, seq, own))
            if what == "both":
                must_precede.append((len(items) - 2, len(items) - 1))
            if what != "missing":
                exp_frames[s, t, :size], exp_sizes[s, t] = (bad if what == "corrupt" else own), size
    assert min(census.values()) >= 3, census
    t2 = int(np.flatnonzero(exp_sizes[1] > 0)[3])
    items += [(1, (base[1] - 1) & 0xFFFF, frames[rows[1], 0, :size]), (2, (base[2] + T) & 0xFFFF, frames[rows[2], 1, :size]), (0, base[0] & 0xFFFF, frames[rows[0], 0, :0]),
              (B, base[0] & 0xFFFF, frames[rows[0], 0, :size]), (-1, 3, frames[rows[0], 1, :size]), (1, (base[1] + t2) & 0xFFFF, exp_frames[1, t2, :size]),
              (1, (base[1] + t2) & 0xFFFF, np.zeros(19 * ch, np.uint8))]       # ... and a copy of a size the geometry refuses: invalid, it loses wherever it stands
    place = rng.permutation(len(items))                            # place[k]: where item k stands in the list
    for a, g in must_precede:
        if place[a] > place[g]:
            place[a], place[g] = place[g], place[a]
    order = np.argsort(place)
    offs, at = np.zeros(len(items), np.int64), 1
    for k in rng.permutation(len(items)):                          # and in the buffer in yet another order, at every alignment
        offs[k] = at
        at += len(items[k][2]) + 1 + k % 3
    buf = np.full(at + (-at % 4), 0xC3, np.uint8)
    for k, (_, _, p) in enumerate(items):
        buf[offs[k]:offs[k] + len(p)] = p
    counts = np.array([T] + [1 + int(np.flatnonzero(exp_sizes[s] > 0).max()) for s in range(1, B)], np.int32)
    assert counts[B - 1] == T - 5
    out = dict(buf=buf, stream=np.array([items[k][0] for k in order], np.int32), seq=np.array([items[k][1] for k in order], np.int32), offsets=offs[order],
               num_bytes=np.array([len(items[k][2]) for k in order], np.int32), base=base.astype(np.int32), floor=np.array([T, 0, -3, 0], np.int32),
               frames=exp_frames, sizes=exp_sizes, counts=counts, size=size, geom_rows=rows)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _oracle(geom):
    """the CPU oracle decoder over each stream's expected sequence, counts[s] frames of it -> [(pcm [c, channels, N], status [c])]"""
    sc = _scenario(geom)
    out = []
    for s, c in enumerate(sc["counts"]):
        o = hf.decode(geom, sc["frames"][:, :c], sc["sizes"][:, :c], np.zeros((len(sc["counts"]), c), np.uint8), rows=[s])
        out.append((o["pcm"][0], o["status"][0]))
    return out


@pytest.mark.parametrize("geom", E2E_GEOMS)
def test_receive_path_without_a_host_wait(dev, geom):
    """probe_device(FULL), ingest_device, set_frame_counts(counts) and decode_device_packed queued on one HIP stream with sync = 0, one wait at the end: the
    tables are the host plan's on the probe's records, and PCM and status equal the oracle decoder on the good copy wherever one exists, the corrupt bytes
    wherever only a corrupt copy exists, a lost frame where neither does; frames behind a stream's count are absent (status 8, no PCM written)"""
    api = _amd().api
    fs, ms, hr, ch, _ = hf.GEOMS[geom]
    sc = _scenario(geom)
    B, T, N, n = len(sc["counts"]), hf.T, hf.frame_len(fs, ms), len(sc["stream"])
    d = _amd().DecBatch(B, fs, ch, ms, hr, None, device=0)
    d_buf, d_stream, d_seq, d_off, d_nb = (dev.put(sc[k]) for k in ("buf", "stream", "seq", "offsets", "num_bytes"))
    d_base, d_floor = dev.put(sc["base"]), dev.put(sc["floor"])
    d_info = dev.put(np.zeros((n, ch, api.FRAME_INFO_WORDS), np.int32))
    d_oo, d_onb, d_ci = dev.put(np.full((B, T), -7, np.int64)), dev.put(np.full((B, T), -7, np.int32)), dev.put(np.full((B, T), -7, np.int32))
    d_counts, d_next, d_stats, d_ist = dev.put(np.full(B, -7, np.int32)), dev.put(np.full(B, -7, np.int32)), dev.put(np.full((B, 4), -7, np.int32)), dev.put(np.full(n, 0xEE, np.uint8))
    d_pcm, d_st = dev.put(np.full((B, T, ch, N), 0x5555, np.int16)), dev.put(np.full((B, T), 0xEE, np.uint8))
    dev.sync()
    s1 = dev.stream()
    d.probe_device(d_buf, sc["buf"].size, d_off, d_nb, sc["size"], n, d_info, api.PROBE_FULL, s1, sync=False)
    d.ingest_device(n, d_stream, d_seq, d_off, d_nb, d_base, T, d_oo, d_onb, d_ci, d_counts, 16, d_info, d_floor, d_next, d_stats, d_ist, s1, sync=False)
    d.set_frame_counts(d_counts)
    d.decode_device_packed(d_buf, sc["buf"].size, d_oo, T, d_pcm, d_onb, sc["size"], None, d_st, 16, s1, sync=False)
    dev.stream_sync(s1)
    # the tables: the host plan on the records the probe wrote
    info = dev.get(d_info, (n, ch, api.FRAME_INFO_WORDS), np.int32)
    want = api.plan_ingest(B, ch, sc["stream"], sc["seq"], sc["offsets"], sc["num_bytes"], sc["base"], T, 16, info, sc["floor"])
    got = dict(offsets=dev.get(d_oo, (B, T), np.int64), num_bytes=dev.get(d_onb, (B, T), np.int32), cell_item=dev.get(d_ci, (B, T), np.int32),
               counts=dev.get(d_counts, (B,), np.int32), next_base=dev.get(d_next, (B,), np.int32), stats=dev.get(d_stats, (B, 4), np.int32),
               item_status=dev.get(d_ist, (n,), np.uint8))
    _same(got, want, geom)
    assert np.array_equal(got["counts"], sc["counts"]) and np.array_equal(got["num_bytes"], sc["sizes"])
    assert np.array_equal(got["next_base"], (sc["base"].astype(np.int64) + sc["counts"]) & 0xFFFF)
    for s in range(B):                                               # each cell's winner holds the bytes the stream is expected to decode
        for t in range(T):
            o, z = int(got["offsets"][s, t]), int(got["num_bytes"][s, t])
            assert np.array_equal(sc["buf"][o:o + z], sc["frames"][s, t, :z]), (s, t)
    ist = got["item_status"]
    for bit in (api.ING_USED, api.ING_DUPLICATE, api.ING_LATE, api.ING_EARLY, api.ING_BAD_STREAM, api.ING_EMPTY, api.ING_REFUSED, api.ING_INVALID):
        assert (ist & bit).any(), bit
    assert (ist == (api.ING_DUPLICATE | api.ING_INVALID)).sum() == 1
    assert ((ist & api.ING_DUPLICATE != 0) & (ist & api.ING_REFUSED != 0)).sum() >= 3            # refused copies that lost against the good one behind them
    assert ((ist & api.ING_USED != 0) & (ist & api.ING_REFUSED != 0)).sum() >= 3                 # ... and sole ones, handed to the decoder as they are
    # the decoder's output
    pcm, st = dev.get(d_pcm, (B, T, ch, N), np.int16), dev.get(d_st, (B, T), np.uint8)
    for s, (wp, ws) in enumerate(_oracle(geom)):
        c = int(sc["counts"][s])
        assert np.array_equal(st[s, :c], ws), (s, st[s].tolist(), ws.tolist())
        bad = np.argwhere((pcm[s, :c] != wp).any(axis=(1, 2)))
        assert len(bad) == 0, (s, "first differing frames", bad[:4].ravel().tolist())
        assert (st[s, c:] == api.DEC_ST_ABSENT).all() and (pcm[s, c:] == 0x5555).all(), s
    d.close()


def test_ingest_is_stateless(dev):
    """decode 13 frames, ingest (the host convenience call, and one more queued with sync = 0 on a second stream), decode the rest: get_state() and num_bytes()
    are what they were before the ingest calls, and the PCM of both decode calls is the oracle's"""
    geom = "48k_10_128B"
    fs, ms, hr, ch, zs = hf.GEOMS[geom]
    frames, sizes, bfi, kind, reason = hf.streams(geom)
    B, T, N = sizes.shape[0], hf.T, hf.frame_len(fs, ms)
    nb, _ = hf.as_empty(sizes, bfi)
    stride = frames.shape[2]
    d = _amd().DecBatch(B, fs, ch, ms, hr, None, device=0)
    c = ref.drawn(99, B, 9, 300, ch, 16, True)
    outs = []
    for a, b in ((0, hf.CUT), (hf.CUT, T)):
        n = b - a
        fr = np.ascontiguousarray(frames[:, a:b])
        po = (np.arange(B * n, dtype=np.int64) * stride).reshape(B, n)
        pcm, st = dev.put(np.zeros((B, n, ch, N), np.int16)), dev.put(np.full((B, n), 0xEE, np.uint8))
        d.decode_device_packed(dev.put(fr), fr.size, dev.put(po), n, pcm, dev.put(np.ascontiguousarray(nb[:, a:b], np.int32)), stride, None, st, sync=True)
        outs.append((dev.get(pcm, (B, n, ch, N), np.int16), dev.get(st, (B, n), np.uint8)))
        if a == 0:
            before = (d.get_state(), [d.num_bytes(s) for s in range(B)])
            want = _plan(c)
            _same(d.ingest(c["stream"], c["seq"], c["offsets"], c["num_bytes"], c["base"], c["n_frames"], c["seq_bits"], c["info"], c["floor"]), want, "ingest()")
            _same(_run(dev, d, c, hip_stream=dev.stream()), want, "second stream")
            after = (d.get_state(), [d.num_bytes(s) for s in range(B)])
            assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    o = hf.decode(geom, frames, sizes, bfi)
    assert np.array_equal(np.concatenate([x[0] for x in outs], axis=1), o["pcm"]) and np.array_equal(np.concatenate([x[1] for x in outs], axis=1) & 1, o["status"])
    d.close()


def test_every_ingest_kernel_ran_under_a_comparison(dev):
    """the sibling library counts its launches: every kernel its code object holds (tools/kernel_resources.py) has run - here, once more, under a comparison, so
    that the test stands alone - and a name it does not hold is answered with -1"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernels
    lib = os.path.join(ROOT, "audio_codec_amd", "liblc3plus_ingest_hip.so")
    names = sorted(kernels(lib, "gfx950"))
    assert names == KERNELS
    c = ref.gpu_lists()["3x4_16_info"]
    d = _batch(c["n_streams"], c["channels"])
    _same(_run(dev, d, c), _plan(c), "3x4_16_info")
    d.close()
    for n in names:
        assert sibling_launches("ingest", n) > 0, n
    assert sibling_launches("ingest", "lc3_probe_side_kernel") == -1
