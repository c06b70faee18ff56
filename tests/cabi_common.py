"""What the C-ABI tests (test_cabi_load.py and the test_*_cabi.py of the extension headers) share: reading a public header, the
host buffer the refusals are driven with, and the check of a ctypes mirror against the header's struct."""
import ctypes
import os
import re

from conftest import REPO


def header(name):
    """the text of include/<name>"""
    return open(os.path.join(REPO, "include", name)).read()


def declarations(text):
    """{entry point: number of parameters} of every declaration in a header's text ((void) = 0)"""
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: 0 if args.strip() == "void" else args.count(",") + 1
            for name, args in re.findall(r"\b(hdlz_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src)}


def host_buffer(size=16384):
    """-> (the object that keeps it alive, a 256-aligned address inside it): host memory, which only a call that is refused may be given"""
    buf = (ctypes.c_uint8 * size)()
    base = ctypes.addressof(buf)
    return buf, base + (-base % 256)


def no_device():
    import torch
    return not torch.cuda.is_available()         # (with a device the good calls would run kernels on host buffers)


def r256(x):
    return (x + 255) // 256 * 256


def check_struct_mirror(header_text, struct, mirror, want):
    """the header's `typedef struct <struct>` has the members `want` ([(C type, name)], uint64_t and uint32_t), and the ctypes class
    `mirror` has them under the same names, of the same sizes, at the offsets a C compiler gives them, and no byte more"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), header_text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+)\s*;", body)
    assert fields == want
    assert [f[0] for f in mirror._fields_] == [f[1] for f in fields]
    assert [ctypes.sizeof(f[1]) for f in mirror._fields_] == [8 if t == "uint64_t" else 4 for t, _ in fields]
    offsets, o = [], 0
    for t, _ in fields:
        offsets.append(o)
        o += 8 if t == "uint64_t" else 4
    assert ctypes.sizeof(mirror) == o and [getattr(mirror, f[1]).offset for f in fields] == offsets
