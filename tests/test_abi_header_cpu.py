"""What scl_amd.lib states by hand against the text of include/scl_hip.h: the flag constants against the #defines, and the field names
of every struct mirror, in declaration order, against the header's typedefs.  Needs neither the library nor a GPU."""
import ctypes
import os
import re

from scl_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "scl_hip.h")).read()


def header_defines():
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(SCL_\w+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))u?\b", HEADER, flags=re.M)}


def test_flag_constants_equal_the_headers_defines():
    defs = header_defines()
    assert defs["SCL_GEMM_C_SPLIT3"] == 0x80000000 and defs["SCL_EINVAL"] == -1      # the reader itself: hexadecimal with a suffix, negative
    flags = [n for n in dir(lib) if n.startswith("GEMM_")]
    assert len(flags) >= 20
    for n in flags:
        if n == "GEMM_C_SPLIT3":      # bit 31: the int32 flag word holds it as a negative number, compared as 32-bit two's complement
            assert -0x80000000 <= lib.GEMM_C_SPLIT3 < 0 and lib.GEMM_C_SPLIT3 + (1 << 32) == defs["SCL_GEMM_C_SPLIT3"]
        else:
            assert getattr(lib, n) == defs["SCL_" + n], n
    shifts = ("ACT_SHIFT", "RMODE_SHIFT", "RACT_SHIFT")
    for n in shifts:
        assert getattr(lib, n) == defs["SCL_GEMM_" + n], n
    # the other direction: every SCL_GEMM_* of the header is bound, but the diagnostic stamp flag, which no Python caller sets
    bound = {"SCL_" + n for n in flags} | {"SCL_GEMM_" + n for n in shifts}
    assert {n for n in defs if n.startswith("SCL_GEMM_")} - bound == {"SCL_GEMM_STAMPS"}
    kids = [n for n in dir(lib) if n.startswith("KID_")]
    assert sorted(kids) == ["KID_AUG", "KID_GEMM", "KID_GEMM_F32"]
    for n in kids:
        assert getattr(lib, n) == defs["SCL_" + n], n
    assert {n for n in defs if n.startswith("SCL_KID_")} - {"SCL_" + n for n in kids} == {"SCL_KID_MAX"}


def header_structs():
    """typedef struct X { ... } X; -> {X: field names in declaration order}: `int64_t bs1, bs2;` and `const float *Wa, *ba;` give a name per
    declarator, `shift[6]` and `lw[8][18]` lose their bounds."""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    out = {}
    for name, body, closing in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        assert name == closing
        out[name] = [re.search(r"([A-Za-z_]\w*)\s*(?:\[[^\]]*\]\s*)*$", decl).group(1)
                     for stmt in body.split(";") if stmt.strip() for decl in stmt.split(",")]
    return out


# The one name a mirror cannot carry: the header's SclRsConv starts with `const float* in`, and `in` is a Python keyword (c.in does not
# parse), so lib.SclRsConv calls that field `inp`.  Same type, same offset 0: the name alone differs.
MIRROR_NAME = {("SclRsConv", "in"): "inp"}


def test_struct_mirrors_list_the_headers_fields_in_order():
    structs = header_structs()
    assert structs["SclOperand"] == ["ptr", "bs1", "bs2", "rbstride", "cout", "rpb", "ld", "cin", "_pad"]      # the reader itself
    assert structs["SclRsConv"][18:21] == ["nvalid", "geom", "shift"] and len(structs["SclRsConv"]) == 29
    assert structs["SclGraphLayer"][4:8] == ["Wa", "ba", "Wb", "bb"] and structs["SclBtseBio"][:2] == ["emb", "lw"]
    assert len(structs) == 15
    for name, fields in structs.items():
        mirror = getattr(lib, name)      # every struct of the header is mirrored
        assert issubclass(mirror, ctypes.Structure)
        assert [f[0] for f in mirror._fields_] == [MIRROR_NAME.get((name, f), f) for f in fields], name
    assert lib.SclRsConv.inp.offset == 0
