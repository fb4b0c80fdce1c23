"""The entry-point table of tests/launch_census.py against the built library, no GPU: the kernels its scenarios claim, together with NOT_REACHED, are exactly
the kernels of the gfx950 code object (tools/kernel_resources.py reads its metadata).  A kernel twin added without a scenario that compares it with the oracle
fails here; tests/test_gpu_launch_census.py shows on the GPU that every scenario launches what it claims."""
import launch_census as lc


def test_table_covers_the_code_object_exactly():
    kernels = set(lc.code_object_kernels())
    assert len(kernels) > 150
    claimed, not_reached = set(lc.claimed()), set(lc.NOT_REACHED)
    assert not claimed & not_reached, sorted(claimed & not_reached)
    assert not (claimed | not_reached) - kernels, ("named in the table, not in the code object", sorted((claimed | not_reached) - kernels))
    assert not kernels - claimed - not_reached, ("kernels without a comparison scenario", sorted(kernels - claimed - not_reached))


def test_every_scenario_is_named_once_and_claims_something():
    names = [s["name"] for s in lc.SCENARIOS]
    assert len(set(names)) == len(names)
    assert all(s["claims"] for s in lc.SCENARIOS)
    assert all(isinstance(why, str) and "lc3_runtime.hip" in why for why in lc.NOT_REACHED.values())


def test_every_kernel_family_has_a_stereo_scenario_with_odd_frames():
    """family: the kernels of one base name (lc3_enc_front4_kernel with its _fmt, _wire, _plc, _rag forms ...).  The utility kernels work on streams, not on
    channels, and the fastmath hook on an array."""
    def family(k):
        return k.split("_kernel")[0]
    stereo = {family(k) for s in lc.SCENARIOS if s["geom"] and s["geom"][3] == 2 for k in s["claims"]}
    odd = [s["name"] for s in lc.SCENARIOS if s["geom"] and s["geom"][3] == 2
           and not any(lc.nbytes_of(s["geom"][0], 2, s["geom"][1], s["geom"][2], r) % 2 for r in s["geom"][4])]
    assert not odd, ("stereo scenarios without an odd stream-frame size", odd)
    mono_only = {family(k) for k in lc.claimed()} - stereo - {"lc3_fastmath_test"}
    assert not mono_only, sorted(mono_only)
