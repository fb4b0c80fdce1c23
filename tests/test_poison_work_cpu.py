"""Poisoned workspaces, no GPU: the classification of tests/poison_work.py held to the source of the host runtime.

The two context structs of audio_codec_amd/csrc/lc3_runtime.hip (and the structs they embed) are parsed from the source text: every pointer member has a class
and a reason, no class names a member that no longer exists, and the members of class `work` are exactly the rows of the runtime's enumerator tables (enc_work,
dec_work), which is what LC3PLUS_POISON_WORK fills and what lc3hip_work_buffer reports.  A buffer added later without a class fails here."""
import ctypes as C
import os

import pytest

import poison_work as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctx", sorted(pw.CLASSES))
def test_every_pointer_member_has_a_class(ctx):
    members, classes = pw.pointer_members(ctx), pw.CLASSES[ctx]
    assert len(members) == len(set(members)), sorted(m for m in members if members.count(m) > 1)
    assert len(members) >= 20, members                               # the parser found the struct, not a fragment of it
    assert sorted(set(members) - set(classes)) == [], "pointer members without a class"
    assert sorted(set(classes) - set(members)) == [], "classes of members that no longer exist"
    for name, (cls, reason) in classes.items():
        assert cls in ("work", "state", "const", "alias", "caller", "host") and len(reason) > 8, name


@pytest.mark.parametrize("ctx", sorted(pw.CLASSES))
def test_the_work_class_is_the_runtimes_table(ctx):
    rows = pw.table(ctx)
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)) and sorted(names) == pw.work_members(ctx)
    assert {r[2] for r in rows} <= {"F32", "I32", "U16", "U8", "I64"}


def test_the_members_the_design_names_as_state_are_state():
    for name in ("d_state", "d_chans", "d_carry", "d_xnext", "ss.d"):
        assert pw.ENC[name][0] == "state", name
    for name in ("d_state", "d_chans", "ss.d"):
        assert pw.DEC[name][0] == "state", name


def test_the_switches_are_read_with_the_other_switches():
    """in read_opts, per batch; LC3PLUS_POISON_CALLS needs LC3PLUS_POISON_WORK"""
    body, _ = pw._body(pw.source(), "static void read_opts(lc3hip_opts* o)")
    assert 'getenv("LC3PLUS_POISON_WORK")' in body and '"LC3PLUS_POISON_CALLS"' in body
    assert "o->poison_calls = o->poison_work ?" in body


def test_the_stub_has_the_two_entries():
    """tools/stub_shim.c mirrors lc3_shim.h: a stub batch has no device buffers, its table is empty"""
    path = os.path.join(ROOT, "audio_codec_amd", "_stub", "liblc3plus_stub.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "audio_codec_amd", "csrc"), "stub"])
    L = C.CDLL(path)
    name, ptr, nbytes, elem = C.c_char_p(), C.c_void_p(), C.c_size_t(), C.c_int()
    for fn in (L.lc3hip_work_buffer, L.lc3hip_dec_work_buffer):
        assert fn(None, 0, C.byref(name), C.byref(ptr), C.byref(nbytes), C.byref(elem)) == 1
