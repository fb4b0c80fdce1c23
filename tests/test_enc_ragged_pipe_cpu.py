"""The ragged forms of the encoder's pipelined kernels (include/lc3plus_batch.h: lc3plus_enc_batch_set_frame_counts; csrc/Makefile: the _epipe objects) in the
built library, from the code-object metadata alone (tools/kernel_resources.py), no GPU: every step of the standard-layout pipeline has its _rag form, no form
uses more scratch than its dense twin or another amount of LDS, and every kernel the library had before them is still there with the figures of the table
committed then (profiles/enc_ragged_resources.txt).  Every comparison is equality, but scratch, which may only shrink."""
import os
import sys

import pytest

from audio_codec_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr   # noqa: E402

VGPR, AGPR, SGPR, SCRATCH, LDS = range(5)
PCM_FORMS = ("", "_fmt", "_wire", "_plc")
# ragged form -> dense twin: the frame-run kernels with their PCM forms, the chains, the frame-per-lane kernels, the two writers
TWINS = {}
for f in PCM_FORMS:
    for k in ("lc3_enc_front4_kernel", "lc3_enc_frontm_kernel", "lc3_enc_front_kernel"):
        TWINS[k + f + "_rag"] = k + f
    TWINS["lc3_enc_resample%s_kernel_rag" % f] = "lc3_enc_resample%s_kernel" % f
for k in ("lc3_enc_hp50_kernel", "lc3_enc_attack_kernel", "lc3_enc_pitch_kernel", "lc3_enc_rate_kernel", "lc3_enc_scf_lane_kernel", "lc3_enc_snsvq_kernel",
          "lc3_enc_shape_lane_kernel", "lc3_enc_shape_lane_kernel_vbw", "lc3_enc_pack_kernel_pk", "lc3_enc_pack_kernel_w5_pk"):
    TWINS[k + "_rag"] = k


@pytest.fixture(scope="module")
def kernels():
    return kr.kernels(api.lib_path(), "gfx950")


def test_every_ragged_pipeline_kernel_exists(kernels):
    assert len(TWINS) == 26
    missing = sorted(k for pair in TWINS.items() for k in pair if k not in kernels)
    assert not missing, missing


@pytest.mark.parametrize("rag", sorted(TWINS))
def test_ragged_form_needs_no_more_than_its_twin(kernels, rag):
    assert rag in kernels and TWINS[rag] in kernels
    r, d = kernels[rag], kernels[TWINS[rag]]
    assert r[SCRATCH] <= d[SCRATCH] and r[LDS] == d[LDS] and r[AGPR] == d[AGPR], (rag, r, d)


def test_every_kernel_of_the_parent_keeps_its_figures(kernels):
    parent = kr.read_table(os.path.join(ROOT, "profiles", "enc_ragged_resources.txt"))
    assert len(parent) == 150
    # the test hook of lc3_fastmath.h got two kinds since that table was written (m_powf(2, x), m_powf(x, k): tests/test_gpu_parity.py::
    # test_device_fastmath_equals_host); it is no kernel of the product, and its figures are pinned here in the table's place
    assert parent["lc3_fastmath_test_kernel"] == (34, 0, 20, 0, 0)
    parent["lc3_fastmath_test_kernel"] = (32, 0, 22, 0, 0)
    changed = {k: (v, kernels.get(k)) for k, v in parent.items() if kernels.get(k) != v}
    assert not changed, changed
    assert sorted(set(kernels) - set(parent)) == sorted(TWINS)            # objects are added, nothing else


def test_committed_table_is_the_library(kernels):
    assert kr.read_table(os.path.join(ROOT, "profiles", "enc_ragged_pipe_resources.txt")) == kernels
