"""The PCM format word of the batch calls on the host alone: exports, the format check and the address rule (lc3plus_pcm_format_check, lc3plus_pcm_offset)."""
import numpy as np
import pytest

import audio_codec_amd
from audio_codec_amd import api

F32, IL, CM = api.PCM_FLOAT32, api.PCM_INTERLEAVED, api.PCM_CHANNEL_MAJOR
TYPES = (16, 24, 32, F32)
LAYOUTS = (0, IL, CM)


def test_symbols_are_exported_and_listed():
    lib = audio_codec_amd.load_library()
    for name in ("lc3plus_pcm_format_check", "lc3plus_pcm_offset"):
        assert name in api.EXPORTS
        assert hasattr(lib, name)


def test_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(api.HERE), "include", "lc3plus_batch.h")).read()
    for name, value in (("LC3PLUS_PCM_FLOAT32", F32), ("LC3PLUS_PCM_INTERLEAVED", IL), ("LC3PLUS_PCM_CHANNEL_MAJOR", CM)):
        m = re.search(r"#define\s+%s\s+(\S+)" % name, text)
        assert m and int(m.group(1), 0) == value


def test_format_check_accepts_every_documented_word():
    lib = audio_codec_amd.load_library()
    for ty in TYPES:
        for lay in LAYOUTS:
            assert lib.lc3plus_pcm_format_check(ty | lay) == 0, (ty, lay)
            assert api.pcm_format(ty, lay) == ty | lay


@pytest.mark.parametrize("word", [0, 8, 17, 16 | IL | CM, F32 | IL | CM, 16 | 0x400, F32 | 0x1000, 16 | F32, 24 | 32, IL, CM, -1, 16 | (1 << 30)])
def test_format_check_rejects(word):
    assert audio_codec_amd.load_library().lc3plus_pcm_format_check(word) != 0


def _all_offsets(fmt, S, T, Cn, N):
    off = np.empty((S, T, Cn, N), dtype=np.int64)
    for s in range(S):
        for t in range(T):
            for c in range(Cn):
                for i in range(N):
                    off[s, t, c, i] = api.pcm_offset(fmt, Cn, T, N, s, t, c, i)
    return off


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("ty", [16, F32])
def test_offsets_are_the_flat_indices_of_the_layouts_array(channels, ty):
    S, T, N = 3, 4, 5
    total = S * T * channels * N
    flat = np.arange(total, dtype=np.int64)
    want = {
        0: flat.reshape(S, T, channels, N),                                                        # [stream][frame][channel][sample]
        IL: flat.reshape(S, T, N, channels).transpose(0, 1, 3, 2),                                 # [stream][time][channel], time = frame * N + sample
        CM: flat.reshape(S, channels, T, N).transpose(0, 2, 1, 3),                                 # [stream][channel][time]
    }
    got = {lay: _all_offsets(ty | lay, S, T, channels, N) for lay in LAYOUTS}
    for lay in LAYOUTS:
        assert (got[lay] == want[lay]).all(), lay
        assert sorted(got[lay].ravel().tolist()) == list(range(total))                             # a bijection onto [0, S T C N)
    if channels == 1:
        assert (got[0] == got[IL]).all() and (got[0] == got[CM]).all()


def test_offset_refuses_arguments_out_of_range():
    assert api.pcm_offset(16, 2, 4, 5, 0, 0, 0, 0) == 0
    for args in ((17, 2, 4, 5, 0, 0, 0, 0), (16, 0, 4, 5, 0, 0, 0, 0), (16, 2, 4, 5, -1, 0, 0, 0), (16, 2, 4, 5, 0, 4, 0, 0), (16, 2, 4, 5, 0, 0, 2, 0),
                 (16, 2, 4, 5, 0, 0, 0, 5), (16 | IL | CM, 2, 4, 5, 0, 0, 0, 0)):
        assert api.pcm_offset(*args) == -1, args


def test_float_inputs_on_the_integer_grids_convert_exactly():
    """What the GPU tests rest on, in float32 arithmetic on the host: x * 32768 for a float sample x on the 16-, 24- or 32-bit grid is the integer path's
    internal sample (int16 as it is, int24 / 256, int32 / 65536), bit for bit."""
    rng = np.random.default_rng(5)
    n = 100000
    i16 = rng.integers(-32768, 32768, n).astype(np.int16)
    assert ((i16.astype(np.float32) / np.float32(32768.0)) * np.float32(32768.0) == i16.astype(np.float32)).all()
    i24 = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int32)
    assert ((i24.astype(np.float32) / np.float32(1 << 23)) * np.float32(32768.0) == i24.astype(np.float32) / np.float32(256.0)).all()
    i32 = rng.integers(-(1 << 23) + 1, 1 << 23, n).astype(np.int32)                               # a quiet signal, finer than the 24-bit grid
    assert ((i32.astype(np.float32) / np.float32(2.0 ** 31)) * np.float32(32768.0) == i32.astype(np.float32) / np.float32(65536.0)).all()


def test_python_shapes_and_dtypes():
    assert api.pcm_shape(16, 2, 3, 2, 5) == (2, 3, 2, 5)
    assert api.pcm_shape(16 | IL, 2, 3, 2, 5) == (2, 15, 2)
    assert api.pcm_shape(F32 | CM, 2, 3, 2, 5) == (2, 2, 15)
    assert api.pcm_dtype(16 | IL) == np.int16 and api.pcm_dtype(24) == np.int32 and api.pcm_dtype(F32 | CM) == np.float32
    assert api.pcm_format(np.float32, "interleaved") == F32 | IL and api.pcm_format(np.int16, "channel_major") == 16 | CM
    with pytest.raises(api.LC3Error):
        api.pcm_format(17)
