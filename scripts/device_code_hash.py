#!/usr/bin/env python3
"""Size and sha256 of every gfx950 code object in the given object files or libraries (default: the built libvspg_hip.so).

    python3 scripts/device_code_hash.py vspg-pbrt-v4_amd/csrc/*.o

The device code of a translation unit is reproducible and does not change when host code or line numbers do, so a refactor that
is meant to leave the kernels alone can show it: run this on the objects before and after and compare the lines.  A unit without
kernels carries no offload bundle and prints "no offload bundle".  The parsing is that of tests/test_headline_scalar_census.py
(_code_objects): uncompressed clang offload bundles.  No GPU needed; nothing is disassembled."""
import hashlib
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(data):
    out = []
    pos = data.find(BUNDLE_MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + 24)
        p = pos + 32
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(BUNDLE_MAGIC, pos + 1)
    return out


def main(paths):
    paths = paths or [os.environ.get("VSPG_LIB") or os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "libvspg_hip.so")]
    for path in paths:
        cos = code_objects(open(path, "rb").read())
        if not cos:
            print("%-28s no offload bundle" % os.path.basename(path))
        for k, co in enumerate(cos):
            print("%-28s #%d %9d bytes  sha256 %s" % (os.path.basename(path), k, len(co), hashlib.sha256(co).hexdigest()))


if __name__ == "__main__":
    main(sys.argv[1:])
