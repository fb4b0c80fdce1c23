"""The ctypes binding against the public headers, no GPU: every function include/lc3.h and include/lc3plus_batch.h declare whose argtypes load_library() sets
takes, position by position, the kind of argument its prototype names, and returns what it names; and the packet layer's parameter tables
(audio_codec_amd/packet.py PARAMS), from which its argtypes and every call of it are made, carry the header's parameter names in the header's order.  Every
comparison is equality."""
import ctypes as C
import os
import re

import pytest

import audio_codec_amd
from audio_codec_amd import api, packet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_TYPES = {"int", "int32_t", "LC3_Error"}                          # ... and every other enum type of the headers (ENUMS)
CTYPE = {"int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t}


def prototypes():
    """{function: (return type, [(parameter type, parameter name)])} of both headers, comments and preprocessor lines stripped: RET NAME(TYPE name, ...);"""
    out = {}
    for header in ("lc3.h", "lc3plus_batch.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
        text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
        for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(lc3\w*)\s*\(([^()]*)\)\s*;", text):
            ps = [re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups() for p in params.split(",") if p.strip() not in ("", "void")]
            out[name] = (" ".join(ret.split()), [(t.strip(), n) for t, n in ps])
    return out


PROTOTYPES = prototypes()
ENUMS = set(re.findall(r"typedef\s+enum\b[^;]*?\}\s*(\w+)\s*;", "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("lc3.h", "lc3plus_batch.h")), flags=re.S))


def kind(ctype):
    """what a C type of the headers is to ctypes; a pointer of any type is a c_void_p"""
    if ctype.endswith("*"):
        return C.c_void_p
    bare = ctype.replace("const ", "").strip()
    if bare in INT_TYPES or bare in ENUMS:
        return C.c_int
    return CTYPE[bare]                                               # KeyError: a type this test does not know - teach it


def bound(argtype):
    """a ctypes argument type as a kind: POINTER(...) counts as a pointer"""
    return C.c_void_p if issubclass(argtype, C._Pointer) else argtype


def test_the_headers_parse():
    """the parser finds the functions: every exported symbol has a prototype, with named parameters"""
    assert len(PROTOTYPES) >= len(api.EXPORTS) and not [s for s in api.EXPORTS if s not in PROTOTYPES]
    assert PROTOTYPES["lc3plus_rtcp_workspace_bytes"] == ("int64_t", [("int64_t", "n_items"), ("int", "n_streams")])
    assert PROTOTYPES["lc3plus_reject_name"] == ("const char*", [("int", "code")])
    assert "LC3_Error" in ENUMS | INT_TYPES


def test_argtypes_and_restypes_agree_with_the_prototypes():
    L = audio_codec_amd.load_library()
    checked = 0
    for name, (ret, params) in PROTOTYPES.items():
        f = getattr(L, name)
        if f.argtypes is not None:
            assert [bound(t) for t in f.argtypes] == [kind(t) for t, _ in params], name
            checked += 1
        if ret == "const char*":
            assert f.restype is C.c_char_p, name
        elif ret.endswith("*"):
            assert f.restype is C.c_void_p, name
        elif ret != "void" and kind(ret) is not C.c_int:
            assert f.restype is kind(ret), name
    assert checked >= 150                                            # what load_library() declared when this test was written


@pytest.mark.parametrize("symbol", sorted(packet.PARAMS))
def test_packet_tables_carry_the_headers_names(symbol):
    """a packet-layer symbol: declared, and its table is the prototype's parameter list by name and by kind"""
    ret, params = PROTOTYPES[symbol]
    f = getattr(audio_codec_amd.load_library(), symbol)
    assert f.argtypes is not None
    assert [n for n, _ in packet.PARAMS[symbol]] == [n for _, n in params]
    assert [packet._CTYPE[k] for _, k in packet.PARAMS[symbol]] == [kind(t) for t, _ in params] == list(f.argtypes)


def test_every_packet_symbol_has_a_table():
    """every exported symbol of the nine packet features is in PARAMS: their batch calls, plans and helpers"""
    features = [s for s in api.EXPORTS if re.search(r"_(probe|ingest|egress|rtp|rtcp|srtp|red|fec)(_|$)", s)]
    assert len(features) >= 40 and set(features) == set(packet.PARAMS)


def test_one_error_class_and_the_names_api_re_exports():
    assert packet.LC3Error is api.LC3Error and packet.load_library is api.load_library
    assert not [n for n in packet.__all__ if getattr(api, n) is not getattr(packet, n)]
    assert api.Batch.red_pack_device is packet._RedPack.red_pack_device and api.DecBatch.probe is packet._Receive.probe
