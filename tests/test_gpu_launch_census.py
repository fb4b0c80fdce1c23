"""Every kernel entry point of the library under an oracle comparison (tests/launch_census.py: SCENARIOS).  One case per scenario: its calls run inside
api.launch_census(), what they wrote is compared with the CPU oracle for equality - never with another GPU path - and every byte a call may not write is checked
untouched; then every entry point the scenario claims must have been launched inside the block, and every name the census reports must be a kernel of the
library's code object.  A later change to the launch decisions cannot leave the table claiming coverage it no longer has."""
import pytest

import launch_census as lc
from test_gpu_dec_varsize_device import _Hip

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("sc", lc.SCENARIOS, ids=[s["name"] for s in lc.SCENARIOS])
def test_scenario_equals_the_oracle_and_launches_what_it_claims(dev, kernels, monkeypatch, tmp_path, sc):
    amd = _amd()
    for k, v in sc.get("env", {}).items():
        monkeypatch.setenv(k, v)                                             # read when the batch is created
    with amd.api.launch_census() as census:
        if sc["kind"] == "enc":
            lc.run_encoder(dev, sc, amd)
        elif sc["kind"] == "dec":
            lc.run_decoder(dev, sc, amd)
        else:
            lc.run_fastmath(tmp_path, amd)
    print(sc["name"], sorted(census.items()))
    missing = [k for k in sc["claims"] if census.get(k, 0) < 1]
    assert not missing, ("claimed, not launched", missing, sorted(census))
    assert set(census) <= kernels, sorted(set(census) - kernels)


def test_the_census_counts_the_launches_of_a_block(dev):
    """the same two calls on two fresh batches: equal counts, one rate kernel and one writer per call; nested blocks each see their own launches; an empty
    block is empty; and lc3hip_launch_census_reset (where no census of the whole process is running, which it would wipe) leaves nothing to read"""
    import ctypes as C
    import os
    amd = _amd()
    sc = next(s for s in lc.SCENARIOS if s["name"] == "pipe_48_stereo")
    with amd.api.launch_census() as a:
        lc.run_encoder(dev, sc, amd)
        with amd.api.launch_census() as inner:
            lc.run_encoder(dev, sc, amd)
    with amd.api.launch_census() as c:
        pass
    assert inner["lc3_enc_rate_kernel"] == 2 and inner["lc3_enc_pack_kernel"] == 2 and c == {}
    assert a == {k: 2 * n for k, n in inner.items()}
    if not os.environ.get("LC3PLUS_LAUNCH_CENSUS"):
        L = amd.load_library()
        L.lc3hip_launch_census_reset()
        L.lc3hip_launch_census_read.restype = C.c_size_t
        assert L.lc3hip_launch_census_read(None, 0) == 1                     # the terminating 0 alone
