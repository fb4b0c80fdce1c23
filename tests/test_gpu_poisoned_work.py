"""GPU: every call reads only what it has written (DESIGN.md "Every workspace word").

The pipelined encoder and the four-kernel decoder hand their work from kernel to kernel through buffers the host runtime keeps from call to call.  A kernel that
reads a word which no kernel of the same call wrote gets, in every other test, zeros from a fresh allocation or the previous call of the same shapes.  Here the
batches are created under LC3PLUS_POISON_WORK (every work buffer filled with typed poison where it is allocated: set A NaN / -1 / all ones, set B 1.5f / 1) and,
where calls need not overlap, LC3PLUS_POISON_CALLS=1 (filled again at the entry of every call), and the existing engines run as they are: equality with the CPU
oracle, untouched sentinels, the claimed entry points launched.  The engines create their batches inside the call, so the switches are set before it.

  a  every encoder and decoder scenario of launch_census.SCENARIOS, sets A and B, poisoned per call
  b  the two promise scenarios once more with the allocation poison alone, so that their calls still overlap
  c  one ordered call-shape sequence per encoder and decoder family (1 ... 273 and 1 ... 129 frames per call on one batch, crossing the one-wave / pipelined switch
     both ways, losses against the call boundaries) poisoned per call, and the promise sequences with the allocation poison alone
  d  the switch reaches the buffers: the runtime's own list (Batch.work_buffers) read back after creation and after one call - poison where the audit says no kernel
     writes (a record's padding words, a row's words behind the spectrum, the rows of a lost frame), none in what the comparison depends on; zeros in the records'
     padding with the switches unset.  Prints, per buffer, the words left unwritten (pytest -s)."""
import numpy as np
import pytest

import call_shapes as cs
import launch_census as lc
from test_gpu_call_shapes import _dec_sequence, _enc_sequence
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu

CODEC = [s for s in lc.SCENARIOS if s["kind"] in ("enc", "dec")]
PROMISE = [s for s in lc.SCENARIOS if s["name"] in ("pipe_48_ready", "dec_48_ready")]
POISON = {np.dtype(np.float32): {"A": 0xFFFFFFFF, "B": 0x3FC00000}, np.dtype(np.int32): {"A": 0xFFFFFFFF, "B": 1}, np.dtype(np.uint16): {"A": 0xFFFF, "B": 1},
          np.dtype(np.uint8): {"A": 0xFF, "B": 1}, np.dtype(np.int64): {"A": 2 ** 64 - 1, "B": 2 ** 64 - 1}}
FR_PADDING = (47, 75)                                                # lc3_plan.h FR_*: the words of a record that belong to no field


def _amd():
    import audio_codec_amd
    return audio_codec_amd


@pytest.fixture
def dev():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def kernels():
    return set(lc.code_object_kernels())


def _poison(monkeypatch, which, calls):
    monkeypatch.setenv("LC3PLUS_POISON_WORK", which)                         # read when a batch is created
    if calls:
        monkeypatch.setenv("LC3PLUS_POISON_CALLS", "1")
    else:
        monkeypatch.delenv("LC3PLUS_POISON_CALLS", raising=False)


def _scenario(dev, kernels, monkeypatch, sc):
    """tests/test_gpu_launch_census.py's case: the engine inside a census, the claims launched"""
    amd = _amd()
    for k, v in sc.get("env", {}).items():
        monkeypatch.setenv(k, v)
    with amd.api.launch_census() as census:
        (lc.run_encoder if sc["kind"] == "enc" else lc.run_decoder)(dev, sc, amd)
    missing = [k for k in sc["claims"] if census.get(k, 0) < 1]
    assert not missing, ("claimed, not launched", missing, sorted(census))
    assert set(census) <= kernels, sorted(set(census) - kernels)


# ---- a, b: the census scenarios ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("sc", CODEC, ids=[s["name"] for s in CODEC])
def test_scenario_poisoned_per_call(dev, kernels, monkeypatch, sc, which):
    _poison(monkeypatch, which, calls=True)
    _scenario(dev, kernels, monkeypatch, sc)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("sc", PROMISE, ids=[s["name"] for s in PROMISE])
def test_promise_scenario_poisoned_at_allocation(dev, kernels, monkeypatch, sc, which):
    """the fill per call waits for the device and so serialises the calls: without it the calls of the promise overlap as they do in a server"""
    _poison(monkeypatch, which, calls=False)
    _scenario(dev, kernels, monkeypatch, sc)


# ---- c: the call-shape sequences --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.ENC_FAMILIES))
def test_encoder_ordered_calls_poisoned_per_call(dev, monkeypatch, name):
    _poison(monkeypatch, "A", calls=True)
    _enc_sequence(dev, name, "enc_ordered")


@pytest.mark.parametrize("name", list(cs.DEC_FAMILIES))
def test_decoder_ordered_calls_poisoned_per_call(dev, monkeypatch, name):
    """through decode_device_sizes: the plan kernel's buffers (sizes, loss and invalid flags) are among the poisoned"""
    _poison(monkeypatch, "A", calls=True)
    _dec_sequence(dev, name, "dec_ordered", "sizes")


@pytest.mark.parametrize("name", list(cs.ENC_READY_FAMILIES))
def test_encoder_under_the_promise_poisoned_at_allocation(dev, monkeypatch, name):
    _poison(monkeypatch, "A", calls=False)
    _enc_sequence(dev, name, "enc_ready", ready=True)


@pytest.mark.parametrize("name", cs.DEC_READY_FAMILIES)
def test_decoder_under_the_promise_poisoned_at_allocation(dev, monkeypatch, name):
    _poison(monkeypatch, "A", calls=False)
    _dec_sequence(dev, name, "dec_ready", "fixed")


# ---- d: the switch reaches the buffers --------------------------------------------------------------------------------------------------------------------------
S, T, FS, MS, N = 3, 12, 48000, 10.0, 480
RATES = (64000, 96000, 40000)                                        # 80, 120 (attack handling), 50 bytes


def _read(dev, bufs, which):
    """{name: (words as unsigned, mask of the words that hold the poison of set `which`)} over the allocated buffers"""
    out = {}
    for name, ptr, nbytes, dt in bufs:
        if ptr:
            w = dev.get(ptr, (nbytes // np.dtype(dt).itemsize,), dt).view("u%d" % np.dtype(dt).itemsize)
            out[name] = (w, w == POISON[np.dtype(dt)][which])
    return out


def _table(side, got):
    for name, (w, p) in got.items():
        print("unwritten %-4s %-12s %9d of %9d words hold poison (%5.1f %%)" % (side, name, int(p.sum()), w.size, 100.0 * p.sum() / max(1, w.size)))


def _pcm():
    return lc.synth_pcm(S, T, N, FS, seed=5)


def test_the_encoders_buffers_hold_poison_where_no_kernel_writes(dev, monkeypatch):
    amd, pcm = _amd(), _pcm()
    plain = amd.Batch(S, FS, 1, MS, 0, list(RATES), device=0)                # created before the switch is set: stays plain
    _poison(monkeypatch, "A", calls=False)
    bat = amd.Batch(S, FS, 1, MS, 0, list(RATES), device=0)
    monkeypatch.delenv("LC3PLUS_POISON_WORK")
    names = [b[0] for b in bat.work_buffers()]
    assert names == [b[0] for b in plain.work_buffers()] and len(names) == len(set(names)) and "d_frec[0]" in names and "d_poff[3]" in names
    made = _read(dev, bat.work_buffers(), "A")
    assert sorted(made) == ["d_cnt"] and made["d_cnt"][1].all()              # what exists after creation: the counts, all poison
    d_in, stride = dev.put(pcm), 128
    outs = [dev.put(np.full((S, T, stride), 0xA5, np.uint8)) for _ in range(2)]
    for b, o in zip((bat, plain), outs):
        b.encode_device(d_in, 16, T, o, stride, sync=True)                   # 12 frames: the pipelined path
    a, p = (dev.get(o, (S, T, stride), np.uint8) for o in outs)
    assert np.array_equal(a, p)                                              # the bytes (and the sentinels behind them) do not depend on the switch
    got, zero = _read(dev, bat.work_buffers(), "A"), _read(dev, plain.work_buffers(), "A")
    _table("enc", got)
    assert sorted(got) == sorted(zero) == ["d_cnt", "d_dumpv[0]", "d_frec[0]", "d_spec[0]", "d_statusv[0]", "d_y12[0]"], sorted(got)
    w = bat.lib.lc3plus_enc_batch_record_words()
    rec, recp = got["d_frec[0]"][0].reshape(S, T, w), got["d_frec[0]"][1].reshape(S, T, w)
    assert recp[:, :, FR_PADDING].all(), "a record's padding words are written by no kernel"
    assert not recp[:, :, :32].any() and not recp[:, :, 76:80].all(axis=2).any(), "scale factors and the rate kernel's words are written in every record"
    left = np.flatnonzero(recp.all(axis=(0, 1))).tolist()
    print("unwritten enc  d_frec[0] words of every record:", left, "of some record:", np.flatnonzero(recp.any(axis=(0, 1))).tolist())
    assert set(FR_PADDING) <= set(left)
    assert not (zero["d_frec[0]"][0].reshape(S, T, w)[:, :, FR_PADDING]).any(), "with the switches unset the padding words are zero (lc3hip_last_records)"
    assert not got["d_statusv[0]"][1].any() and not got["d_statusv[0]"][0].any()     # cleared per call, no status bit set
    ylen, srow = 400, 512                                                    # 48 kHz / 10 ms: 400 lines and 100 band energies in rows of 512 words, tiled by 16 (lc3_plan.h LC3D_SROW)
    specp = got["d_spec[0]"][1].reshape(S, srow // 16, T, 16).transpose(0, 2, 1, 3).reshape(S, T, srow)
    assert not specp[:, :, :ylen + ylen // 4].any() and specp[:, :, ylen + ylen // 4:].all(), "a row's spectrum and energies are written, its 12 words of rounding are not"
    dump = got["d_dumpv[0]"][1]
    assert 0 < dump.sum() < dump.size                                        # the writer's scratch: scalars, residual words and spectrum up to lastnz; the rest is nobody's
    assert not got["d_y12[0]"][1].any(), "128 words per frame at 12.8 kHz x 10 ms: the resampler writes every word"
    assert got["d_cnt"][1].all()                                             # no ragged call was made
    bat.close()
    plain.close()


def test_the_decoders_buffers_hold_poison_where_no_kernel_writes(dev, monkeypatch):
    amd, pcm = _amd(), _pcm()
    enc = amd.Batch(S, FS, 1, MS, 0, list(RATES), device=0)
    frames = enc.encode(pcm)                                                 # [S, T, stride]
    nbytes = [enc.num_bytes(s) for s in range(S)]
    enc.close()
    _poison(monkeypatch, "A", calls=False)
    d = amd.DecBatch(S, FS, 1, MS, 0, None, device=0)
    monkeypatch.delenv("LC3PLUS_POISON_WORK")
    made = _read(dev, d.work_buffers(), "A")
    assert sorted(made) == ["d_cnt"] and made["d_cnt"][1].all()
    nb = np.repeat(np.array(nbytes, np.int32)[:, None], T, axis=1)
    bfi = np.zeros((S, T), np.uint8)
    bfi[1, 4] = 1                                                            # one lost frame: no parsed row
    stride = frames.shape[2]
    d_pcm, d_st = dev.put(np.full((S, T, N), 0x5A5A, np.uint16)), dev.put(np.full((S, T), 0xEE, np.uint8))
    d.decode_device_sizes(dev.put(frames), stride, T, d_pcm, dev.put(nb), dev.put(bfi), d_st, sync=True)
    got = _read(dev, d.work_buffers(), "A")
    _table("dec", got)
    assert sorted(got) == ["d_bfi", "d_cnt", "d_inval", "d_ov", "d_rec", "d_sizes", "d_ws"], sorted(got)
    for name in ("d_bfi", "d_inval", "d_sizes"):
        assert not got[name][1].any(), (name, "the plan kernel writes every entry")
    assert np.array_equal(got["d_bfi"][0].reshape(S, T), bfi) and np.array_equal(got["d_sizes"][0].reshape(S, T), np.where(bfi, 0, nb))
    ylen, wsr = 400, 480                                                     # 48 kHz / 10 ms: 400 spectral lines in rows of 480 words
    rowp = got["d_ws"][1].reshape(S, wsr // 16, T, 16).transpose(0, 2, 1, 3).reshape(S, T, wsr)      # lc3_plan.h LC3D_ROW_BASE / LC3D_ROW_OFF: tiled by 16 words
    good = bfi == 0
    assert not rowp[good][:, :ylen].any(), "a good frame's row is written up to the spectrum's length by the parser's second sweep"
    assert rowp[good][:, ylen:].all(), "... and no further"
    assert rowp[~good].all(), "a lost frame has no parsed row"
    recp = got["d_rec"][1].reshape(S, T, 112)
    assert not recp[:, :, :40].all(axis=2).any() and recp[good][:, 40:44].all(), "a good frame's four concealment words are written by no kernel"
    assert got["d_rec"][0].reshape(S, T, 112)[1, 4, 39] == 1 and not recp[1, 4, 40:44].all()      # the lost frame: bfi, and its concealment words written
    ovp = got["d_ov"][1].reshape(S, T, 480)
    assert not ovp.any(), "N = 480: the IMDCT writes the whole row, of a lost frame too"
    st = dev.get(d_st, (S, T), np.uint8)
    assert st[1, 4] != 0 and not st[good].any()
    d.close()
