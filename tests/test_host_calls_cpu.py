"""The host code of the batches (audio_codec_amd/csrc/lc3_host.c) against its recorded behaviour, without a GPU: tests/golden/make_golden_host_calls.py runs a table
of refusals (every public batch and sharded entry, every plan hook: each bad argument and each pair of them) and a list of call sequences against the build whose
HIP side is tools/stub_shim.c, and tests/golden/host_calls.json holds what they gave: return codes, the stub's two logs (launches and configuration traffic) and the
getters afterwards.  The replay here must give the file again.  Every comparison is equality."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def replay():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "audio_codec_amd", "csrc"), "stub"])
    spec = importlib.util.spec_from_file_location("make_golden_host_calls", os.path.join(GOLDEN, "make_golden_host_calls.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "host_calls.json")) as f:
        text = f.read()
    return gen, gen.generate(), text


def _differences(got, want):
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_the_file_covers_what_it_is_meant_to(replay):
    gen, _, text = replay
    want = json.loads(text)
    rows = gen.refusal_rows(want)
    assert len(rows) == 3 * len(gen.entries(gen.Bufs(gen.GEOMS["mono"])))
    for g in gen.GEOMS:                                              # every geometry: the batch calls, the sharded calls, the hooks
        for name in ("enc_batch_encode", "enc_batch_encode_bitrates", "enc_batch_encode_bandwidths", "enc_batch_encode_rates_device", "enc_batch_encode_packed",
                     "dec_batch_decode", "dec_batch_decode_sizes", "dec_batch_decode_sizes_device", "dec_batch_decode_packed", "enc_sharded_encode",
                     "dec_sharded_decode", "enc_sharded_num_bytes", "enc_sharded_bandwidth", "dec_sharded_num_bytes", "enc_batch_create", "dec_batch_create",
                     "enc_sharded_create", "dec_sharded_create", "enc_plan_bandwidths", "enc_plan_bitrates", "enc_plan_rates_lenient", "enc_plan_rates_ragged",
                     "plan_chan", "dec_plan_sizes", "dec_plan_sizes_lenient", "dec_plan_packed_lenient", "frame_info_side", "stream_state_header_enc",
                     "stream_state_header_dec", "enc_batch_reset_streams", "dec_batch_import_streams"):
            row = rows["%s %s" % (g, name)]
            assert "good" in row and any(" & " in k for k in row), (g, name)
    assert rows["mono dec_sharded_num_bytes"]["stream_high"] == 0 and rows["mono enc_sharded_bandwidth"]["stream_high"] == -1
    assert rows["hr96 enc_batch_encode_bandwidths"]["good"] == rows["hr96 enc_plan_bandwidths"]["good"] != 0       # LC3_HRMODE_BW_ERROR
    assert len(want["scripts"]) == 60 and all(k.split()[0] in ("mono", "stereo") for k in want["scripts"])


def test_refusals_are_the_recorded_ones(replay):
    gen, got, text = replay
    want, got = gen.refusal_rows(json.loads(text)), gen.refusal_rows(got)
    bad = _differences(got, want)
    detail = {k: {c: (got.get(k, {}).get(c), want.get(k, {}).get(c)) for c in _differences(got.get(k, {}), want.get(k, {}))} for k in bad[:5]}
    assert not bad, ("rows that differ (case: got, recorded)", len(bad), detail)


def test_scripts_are_the_recorded_ones(replay):
    gen, got, text = replay
    want = json.loads(text)["scripts"]
    bad = _differences(got["scripts"], want)
    detail = {k: {p: (got["scripts"].get(k, {}).get(p), want.get(k, {}).get(p)) for p in _differences(got["scripts"].get(k, {}), want.get(k, {}))} for k in bad[:2]}
    assert not bad, ("scripts that differ (part: got, recorded)", len(bad), detail)


def test_the_file_is_what_the_generator_writes(replay):
    gen, got, text = replay
    assert gen.dumps(got) == text
