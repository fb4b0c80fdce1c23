"""GPU tests of the sharded batches (lc3plus_{enc,dec}_sharded_*, api.ShardedBatch / api.ShardedDecBatch): a sharded batch gives exactly what one unsharded
batch of the same streams gives, which is what the CPU oracle gives - every comparison is equality of bytes, samples or codes.  devices = [0, 0] (two
shards, two contexts, one device) unless a test says otherwise, so the file runs on a one-GPU machine; the last test wants a second device.  Also here: two
host threads driving two plain batches at once, which the boundary has always claimed to allow."""
import threading

import numpy as np
import pytest

from lc3_harness import Oracle, make_dec_case, oracle_decode_streams, oracle_encode_streams, synth_pcm
from test_gpu_dec_varsize_device import _Hip
from test_gpu_multidevice import _ndev

pytestmark = pytest.mark.gpu
LC3_BITRATE_ERROR, LC3_BW_WARNING = 6, 18


def _amd():
    import audio_codec_amd
    return audio_codec_amd


def _rates(S, base=(64000, 32000, 128000)):
    return [base[i % len(base)] for i in range(S)]


def _same_as_oracle(got, want, a=0):
    """got uint8 [S, T, stride] against the oracle's frames want[s] [T_all, nbytes] from frame a."""
    T = got.shape[1]
    for s, w in enumerate(want):
        bad = np.argwhere((got[s, :, :w.shape[1]] != w[a:a + T]).any(axis=1))
        assert len(bad) == 0, ("stream", s, "first differing frames", bad[:4].ravel().tolist())


def _oracle_multi(pcm, fs, ms, hr, rates):
    """pcm [S, T, channels, N] -> list of [T, nbytes]"""
    outs = []
    for s in range(pcm.shape[0]):
        o = Oracle(fs, pcm.shape[2], ms, hr, int(rates[s]), True)
        outs.append(np.stack([o.encode(pcm[s, t]) for t in range(pcm.shape[1])]))
    return outs


def _close(*xs):
    for x in xs:
        x.close()


# ---- 7. encoder equals unsharded equals oracle ----
@pytest.mark.parametrize("S,devices", [(33, [0, 0]), (7, [0, 0, 0])])
def test_encoder_equals_unsharded_equals_oracle(S, devices):
    fs, ms, N = 48000, 10.0, 480
    rates = _rates(S)
    pcm = synth_pcm(S, 44, N, fs, seed=21)
    want = oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True)
    sb = _amd().ShardedBatch(S, fs, 1, ms, 0, rates, devices)
    ub = _amd().Batch(S, fs, 1, ms, 0, rates, device=0)
    try:
        assert sb.n_shards == len(devices) and sb.stride == ub.stride and sb.state_size == ub.get_state().size
        assert [c for _, c in sb.blocks] == ([17, 16] if S == 33 else [3, 2, 2])
        a = 0
        for T in (4, 40):                                            # the one-wave kernel, then the pipelined path
            got, ref = sb.encode(pcm[:, a:a + T]), ub.encode(pcm[:, a:a + T])
            assert got.shape == ref.shape and (got == ref).all()
            _same_as_oracle(got, want, a)
            assert all(sb.last_kernel_ms(i) > 0 for i in range(sb.n_shards))
            a += T
    finally:
        _close(sb, ub)


def test_stereo_and_float32_interleaved():
    fs, ms, N, S, ch = 16000, 10.0, 160, 9, 2
    rates = _rates(S, (64000, 48000, 96000))
    pcm = synth_pcm(S * ch, 24, N, fs, seed=22).reshape(S, ch, 24, N).transpose(0, 2, 1, 3).copy()
    want = _oracle_multi(pcm, fs, ms, 0, rates)
    sb = _amd().ShardedBatch(S, fs, ch, ms, 0, rates, [0, 0])
    sf = _amd().ShardedBatch(S, fs, ch, ms, 0, rates, [0, 0])
    ub = _amd().Batch(S, fs, ch, ms, 0, rates, device=0)
    try:
        a = 0
        for T in (4, 20):
            x = pcm[:, a:a + T]
            got, ref = sb.encode(x), ub.encode(x)
            assert (got == ref).all()
            _same_as_oracle(got, want, a)
            xf = (x.transpose(0, 1, 3, 2).reshape(S, T * N, ch) / 32768.0).astype(np.float32)      # [stream][time][channel], full scale 1.0
            assert (sf.encode(xf, layout="interleaved") == ref).all()
            a += T
    finally:
        _close(sb, sf, ub)


def test_high_resolution():
    fs, ms, N, S = 48000, 5.0, 240, 7
    rates = _rates(S, (160000, 200000, 256000))
    pcm = synth_pcm(S, 24, N, fs, seed=23)
    want = oracle_encode_streams(pcm, fs, ms, 1, rates, portable_math=True)
    sb = _amd().ShardedBatch(S, fs, 1, ms, 1, rates, [0, 0])
    ub = _amd().Batch(S, fs, 1, ms, 1, rates, device=0)
    try:
        a = 0
        for T in (4, 20):
            got, ref = sb.encode(pcm[:, a:a + T]), ub.encode(pcm[:, a:a + T])
            assert (got == ref).all()
            _same_as_oracle(got, want, a)
            a += T
    finally:
        _close(sb, ub)


# ---- 8. per-frame rates and bandwidths ----
def test_per_frame_rates_and_bandwidths():
    fs, ms, N, S, T = 48000, 10.0, 480, 33, 12
    rates = _rates(S)
    rng = np.random.RandomState(8)
    pcm = synth_pcm(S, 5 * T, N, fs, seed=24)
    br = rng.choice([32000, 64000, 96000, 128000], size=(S, T)).astype(np.int32)
    bw = rng.choice([0, 4000, 8000, 16000, 20000], size=(S, T)).astype(np.int32)
    sb = _amd().ShardedBatch(S, fs, 1, ms, 0, rates, [0, 0])
    ub = _amd().Batch(S, fs, 1, ms, 0, rates, device=0)
    try:
        a = 0
        for kw in (dict(bitrates=br), dict(bandwidths=bw), dict(bitrates=br[::-1].copy(), bandwidths=bw)):
            got, ref = sb.encode(pcm[:, a:a + T], **kw), ub.encode(pcm[:, a:a + T], **kw)
            assert got.shape == ref.shape and (got == ref).all() and (sb.last_num_bytes == ub.last_num_bytes).all()
            assert sb.last_result == 0 and ub.last_result == 0
            assert [sb.num_bytes(s) for s in range(S)] == [ub.num_bytes(s) for s in range(S)]
            assert [sb.bandwidth(s) for s in range(S)] == [ub.bandwidth(s) for s in range(S)]
            a += T
        # a bandwidth set_bandwidth refuses, in the second shard only: the call does all its work and returns the warning
        assert sb.owner(20)[0] == 1
        refused = bw.copy(); refused[20, 3] = 24000
        got, ref = sb.encode(pcm[:, a:a + T], bandwidths=refused), ub.encode(pcm[:, a:a + T], bandwidths=refused)
        assert sb.last_result == LC3_BW_WARNING and ub.last_result == LC3_BW_WARNING and (got == ref).all()
        a += T
        # a bad rate in the second shard only: refused, and nothing ran on either shard - the next plain call continues as the unsharded batch,
        # which never saw the refused call
        bad = br.copy(); bad[25, 5] = 1000
        with pytest.raises(_amd().LC3Error) as e:
            sb.encode(pcm[:, a:a + T], bitrates=bad)
        assert e.value.code == LC3_BITRATE_ERROR
        got, ref = sb.encode(pcm[:, a:a + T]), ub.encode(pcm[:, a:a + T])
        assert (got == ref).all()
    finally:
        _close(sb, ub)


# ---- 9. device pointers ----
def _on(dev, device):
    assert dev.hip.hipSetDevice(device) == 0


def test_device_pointers_sync0_and_input_ready():
    fs, ms, N, S, T = 48000, 10.0, 480, 33, 12
    rates = _rates(S)
    pcm = synth_pcm(S, 4 * T, N, fs, seed=25)
    want = oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True)
    sb = _amd().ShardedBatch(S, fs, 1, ms, 0, rates, [0, 0])
    dev = _Hip()
    try:
        stride = sb.stride

        def queue(a):
            d_pcm, d_out = [], []
            for i, (first, count) in enumerate(sb.blocks):       # each shard's block on its own device
                _on(dev, sb.devices[i])
                d_pcm.append(dev.put(pcm[first:first + count, a:a + T])); d_out.append(dev.zeros(count * T * stride))
            return d_pcm, d_out

        def fetch(d_out):
            for i in range(sb.n_shards):                             # one synchronise per shard
                _on(dev, sb.devices[i]); dev.sync()
            return np.concatenate([dev.get(d_out[i], (count, T, stride), np.uint8) for i, (_, count) in enumerate(sb.blocks)])

        d_pcm, d_out = queue(0)
        sb.encode_device(d_pcm, 16, T, d_out, stride, sync=False)
        _same_as_oracle(fetch(d_out), want, 0)
        # three calls back to back under the input-ready promise on every shard: every buffer complete before the first call
        for i in range(sb.n_shards):
            sb.shard(i).set_input_ready(1)
        bufs = [queue(T * k) for k in (1, 2, 3)]
        for i in range(sb.n_shards):
            _on(dev, sb.devices[i]); dev.sync()
        for d_pcm, d_out in bufs:
            sb.encode_device(d_pcm, 16, T, d_out, stride, sync=False)
        for k, (_, d_out) in enumerate(bufs):
            _same_as_oracle(fetch(d_out), want, T * (k + 1))
        _on(dev, 0)
    finally:
        dev.free()
        sb.close()


# ---- 10. state ----
def test_state_moves_between_unsharded_two_and_three_shards():
    fs, ms, N, S, T = 48000, 10.0, 480, 33, 12
    rates = _rates(S)
    pcm = synth_pcm(S, 3 * T, N, fs, seed=26)
    want = oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True)
    A = _amd()
    ub, whole = A.Batch(S, fs, 1, ms, 0, rates, device=0), A.Batch(S, fs, 1, ms, 0, rates, device=0)
    s2, s3 = A.ShardedBatch(S, fs, 1, ms, 0, rates, [0, 0]), A.ShardedBatch(S, fs, 1, ms, 0, rates, [0, 0, 0])
    try:
        assert s2.state_size == s3.state_size == ub.get_state().size
        parts = [ub.encode(pcm[:, :T])]
        s2.set_state(ub.get_state())
        parts.append(s2.encode(pcm[:, T:2 * T]))
        s3.set_state(s2.get_state())
        parts.append(s3.encode(pcm[:, 2 * T:]))
        got = np.concatenate(parts, axis=1)
        assert (got == np.concatenate([whole.encode(pcm[:, k * T:(k + 1) * T]) for k in range(3)], axis=1)).all()
        _same_as_oracle(got, want)
    finally:
        _close(ub, whole, s2, s3)


# ---- 11. lifecycle through a borrowed shard ----
def test_reset_one_stream_through_a_borrowed_shard():
    fs, ms, N, S, T = 48000, 10.0, 480, 33, 12
    rates = _rates(S)
    pcm = synth_pcm(S, 2 * T, N, fs, seed=27)
    want = oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True)
    fresh = oracle_encode_streams(pcm[20:21, T:], fs, ms, 0, rates[20:21], portable_math=True)[0]      # a new encoder from the first new frame
    sb = _amd().ShardedBatch(S, fs, 1, ms, 0, rates, [0, 0])
    try:
        _same_as_oracle(sb.encode(pcm[:, :T]), want, 0)
        k, local = sb.owner(20)
        assert (k, local) == (1, 3)
        sb.shard(k).reset_streams([local])
        got = sb.encode(pcm[:, T:])
        assert (got[20, :, :fresh.shape[1]] == fresh).all()
        for s in range(S):
            if s != 20:
                assert (got[s, :, :want[s].shape[1]] == want[s][T:]).all(), s
    finally:
        sb.close()


# ---- 12. the decoder twin ----
def test_decoder_twin():
    fs, ms, N, S, T = 48000, 10.0, 480, 9, 12
    rates = _rates(S)
    frames, nbytes, bfi = make_dec_case(fs, ms, 0, 1, rates, 3 * T, seed=12)
    want, wst = oracle_decode_streams(frames, nbytes, bfi, fs, ms, 0, 1)
    A = _amd()
    ud = A.DecBatch(S, fs, 1, ms, 0, nbytes, device=0)
    s2, s3 = A.ShardedDecBatch(S, fs, 1, ms, 0, nbytes, [0, 0]), A.ShardedDecBatch(S, fs, 1, ms, 0, nbytes, [0, 0, 0])
    dev = _Hip()
    try:
        assert s2.state_size == s3.state_size == ud.get_state().size and s2.delay > 0 and s2.blocks == [(0, 5), (5, 4)]
        # decode with bfi, and the state handed from the unsharded batch to two shards to three
        p0, t0 = ud.decode(frames[:, :T], bfi[:, :T])
        s2.set_state(ud.get_state())
        p1, t1 = s2.decode(frames[:, T:2 * T], bfi[:, T:2 * T])
        s3.set_state(s2.get_state())
        p2, t2 = s3.decode(frames[:, 2 * T:], bfi[:, 2 * T:])
        assert (np.concatenate([p0, p1, p2], axis=1) == want).all() and (np.concatenate([t0, t1, t2], axis=1) == wst).all()
        # per-frame sizes: 0 = lost
        A2 = A.ShardedDecBatch(S, fs, 1, ms, 0, nbytes, [0, 0]); U2 = A.DecBatch(S, fs, 1, ms, 0, nbytes, device=0)
        nb = np.where(bfi == 1, 0, np.asarray(nbytes, np.int32)[:, None]).astype(np.int32)
        got, st = A2.decode(frames, num_bytes=nb)
        ref, rst = U2.decode(frames, num_bytes=nb)
        assert (got == ref).all() and (st == rst).all() and (got == want).all() and (st == wst).all()
        _close(A2, U2)
        # device pointers, one per shard; no flags on this path
        want_clean, wst_clean = oracle_decode_streams(frames[:, :T], nbytes, None, fs, ms, 0, 1)
        A3 = A.ShardedDecBatch(S, fs, 1, ms, 0, nbytes, [0, 0])
        d_fr, d_pcm = [], []
        for i, (first, count) in enumerate(A3.blocks):
            _on(dev, A3.devices[i])
            d_fr.append(dev.put(frames[first:first + count, :T])); d_pcm.append(dev.zeros(count * T * N * 2))
        A3.decode_device(d_fr, frames.shape[2], T, d_pcm, sync=False)
        for i in range(A3.n_shards):
            _on(dev, A3.devices[i]); dev.sync()
        got = np.concatenate([dev.get(d_pcm[i], (count, T, 1, N), np.int16) for i, (_, count) in enumerate(A3.blocks)])
        assert (got == want_clean).all()
        A3.decode_device(d_fr, frames.shape[2], T, d_pcm, sync=True)       # and waited for inside the call
        _on(dev, 0)
        A3.close()
    finally:
        dev.free()
        _close(ud, s2, s3)


# ---- 13. two host threads, two plain batches ----
def _run_together(jobs, timeout=600):
    """Starts one thread per job behind a barrier; a thread that is still running after `timeout` seconds ends the whole run (nothing more may be started on
    a device whose call is stuck)."""
    barrier = threading.Barrier(len(jobs))
    errors = [None] * len(jobs)

    def main(i):
        try:
            barrier.wait(timeout=60)
            jobs[i]()
        except BaseException as e:                                   # noqa: BLE001 - reported by the test
            errors[i] = e
    threads = [threading.Thread(target=main, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    if any(t.is_alive() for t in threads):
        pytest.exit("a thread is stuck inside a batch call", returncode=3)
    assert errors == [None] * len(jobs), errors


CUTS = [4, 24] * 25                                                  # 50 calls of alternating 4 and 24 frames


def test_two_threads_two_batches():
    fs, ms, N, S = 48000, 10.0, 480, 4
    T = sum(CUTS)
    A = _amd()
    pcms = [synth_pcm(S, T, N, fs, seed=31), synth_pcm(S, T, N, fs, seed=32)]
    rates = [_rates(S), _rates(S, (96000, 64000))]
    batches = [A.Batch(S, fs, 1, ms, 0, rates[i], device=0) for i in range(2)]
    outs = [[], []]

    def job(i):
        def run():
            a = 0
            for n in CUTS:
                outs[i].append(batches[i].encode(pcms[i][:, a:a + n])); a += n
        return run
    try:
        _run_together([job(0), job(1)])
        for i in range(2):
            _same_as_oracle(np.concatenate(outs[i], axis=1), oracle_encode_streams(pcms[i], fs, ms, 0, rates[i], portable_math=True))
    finally:
        _close(*batches)


def test_two_threads_one_encoder_one_decoder():
    fs, ms, N, S = 48000, 10.0, 480, 4
    T = sum(CUTS)
    A = _amd()
    pcm, rates = synth_pcm(S, T, N, fs, seed=33), _rates(S)
    frames, nbytes, bfi = make_dec_case(fs, ms, 0, 1, _rates(S, (64000, 96000)), T, seed=13)
    enc, dec = A.Batch(S, fs, 1, ms, 0, rates, device=0), A.DecBatch(S, fs, 1, ms, 0, nbytes, device=0)
    out, dout, dst = [], [], []

    def encode():
        a = 0
        for n in CUTS:
            out.append(enc.encode(pcm[:, a:a + n])); a += n

    def decode():
        a = 0
        for n in CUTS:
            p, s = dec.decode(frames[:, a:a + n], bfi[:, a:a + n]); dout.append(p); dst.append(s); a += n
    try:
        _run_together([encode, decode])
        _same_as_oracle(np.concatenate(out, axis=1), oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True))
        want, wst = oracle_decode_streams(frames, nbytes, bfi, fs, ms, 0, 1)
        assert (np.concatenate(dout, axis=1) == want).all() and (np.concatenate(dst, axis=1) == wst).all()
    finally:
        _close(enc, dec)


# ---- 14. a real second device ----
@pytest.mark.skipif(_ndev() < 2, reason="needs two visible devices")
def test_two_real_devices_and_a_checkpoint_across_them():
    fs, ms, N, S = 48000, 10.0, 480, 33
    rates = _rates(S)
    pcm = synth_pcm(S, 56, N, fs, seed=21)
    want = oracle_encode_streams(pcm, fs, ms, 0, rates, portable_math=True)
    a01, a10 = _amd().ShardedBatch(S, fs, 1, ms, 0, rates, [0, 1]), _amd().ShardedBatch(S, fs, 1, ms, 0, rates, [1, 0])
    try:
        assert a01.devices == [0, 1] and a10.devices == [1, 0]
        _same_as_oracle(a01.encode(pcm[:, :4]), want, 0)
        _same_as_oracle(a01.encode(pcm[:, 4:44]), want, 4)
        a10.set_state(a01.get_state())                               # the checkpoint taken on [0, 1] resumes on [1, 0]
        _same_as_oracle(a10.encode(pcm[:, 44:]), want, 44)
    finally:
        _close(a01, a10)
