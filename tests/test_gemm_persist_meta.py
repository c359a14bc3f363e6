"""The persistent wide-tile GEMM kernels of the BUILT library (scl_gemm_persist_w8_kernel, gemm_w8.hip) have no private segment and spill no
register.  A kernel with scratch between kernels without it costs a queue-side scratch set-up per dispatch (0.5 ms each: the round-3
form of this kernel made the train step 84.8 instead of 47.4 ms), so such a kernel must not ship.  Read from the code objects' metadata
notes only (NT_AMDGPU_METADATA, a msgpack map) — no compiler, no GPU."""
import struct

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _unpack(b, i):
    """Minimal msgpack reader: (value, next offset)."""
    t = b[i]
    if t <= 0x7F:
        return t, i + 1
    if t >= 0xE0:
        return t - 0x100, i + 1
    if 0x80 <= t <= 0x8F or t in (0xDE, 0xDF):
        n, i = (t & 0xF, i + 1) if t <= 0x8F else ((struct.unpack_from(">H", b, i + 1)[0], i + 3) if t == 0xDE else (struct.unpack_from(">I", b, i + 1)[0], i + 5))
        out = {}
        for _ in range(n):
            k, i = _unpack(b, i)
            out[k], i = _unpack(b, i)
        return out, i
    if 0x90 <= t <= 0x9F or t in (0xDC, 0xDD):
        n, i = (t & 0xF, i + 1) if t <= 0x9F else ((struct.unpack_from(">H", b, i + 1)[0], i + 3) if t == 0xDC else (struct.unpack_from(">I", b, i + 1)[0], i + 5))
        out = []
        for _ in range(n):
            v, i = _unpack(b, i)
            out.append(v)
        return out, i
    if 0xA0 <= t <= 0xBF:
        n = t & 0x1F
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if t in (0xD9, 0xDA, 0xDB, 0xC4, 0xC5, 0xC6):
        w = {0xD9: 1, 0xDA: 2, 0xDB: 4, 0xC4: 1, 0xC5: 2, 0xC6: 4}[t]
        n = int.from_bytes(b[i + 1:i + 1 + w], "big")
        raw = b[i + 1 + w:i + 1 + w + n]
        return (raw.decode() if t >= 0xD9 else raw), i + 1 + w + n
    if t == 0xC0:
        return None, i + 1
    if t in (0xC2, 0xC3):
        return t == 0xC3, i + 1
    fixed = {0xCC: (">B", 1), 0xCD: (">H", 2), 0xCE: (">I", 4), 0xCF: (">Q", 8), 0xD0: (">b", 1), 0xD1: (">h", 2), 0xD2: (">i", 4),
             0xD3: (">q", 8), 0xCA: (">f", 4), 0xCB: (">d", 8)}
    if t in fixed:
        f, w = fixed[t]
        return struct.unpack_from(f, b, i + 1)[0], i + 1 + w
    raise ValueError("msgpack type 0x%02x" % t)


def _code_objects(data):
    """The gfx950 code objects (ELF images) of every offload bundle in the library."""
    pos = data.find(BUNDLE_MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        o = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tlen]
            o += 24 + tlen
            if b"gfx950" in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(BUNDLE_MAGIC, pos + 1)


def _kernel_metadata(elf):
    """The amdhsa.kernels list of one code object, from its NT_AMDGPU_METADATA note."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for s in range(shnum):
        _, stype, _, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + s * shentsize)
        if stype != 7:      # SHT_NOTE
            continue
        p, end = off, off + size
        while p + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            name = elf[p + 12:p + 12 + namesz]
            d0 = p + 12 + (namesz + 3) // 4 * 4
            if ntype == 32 and name.rstrip(b"\0") == b"AMDGPU":
                return _unpack(elf[d0:d0 + descsz], 0)[0].get("amdhsa.kernels", [])
            p = d0 + (descsz + 3) // 4 * 4
    return []


def test_persistent_gemm_kernels_have_no_private_segment_and_no_spills():
    from scl_amd import lib
    data = open(lib.LIB_PATH, "rb").read()
    seen = []
    for elf in _code_objects(data):
        for k in _kernel_metadata(elf):
            if "scl_gemm_persist_w8_kernel" not in k[".name"]:
                continue
            seen.append(k[".name"])
            assert k[".private_segment_fixed_size"] == 0, k[".name"]
            assert k[".vgpr_spill_count"] == 0, k[".name"]
            assert not k.get(".uses_dynamic_stack", False), k[".name"]
    # 208-row tiles: epilogue kinds 1, 2, 5 x K-contiguous / transposed B; 256-row tiles: conv forward (NN, kind 5), conv data gradient (NT, kind 1)
    assert len(seen) == 8, seen
