"""A test-side OpenEXR writer and reader (struct, zlib, NumPy) for the subset of the container the host's image layer covers.
Written from the container's layout, not from host/vspg_image.cpp: the two are checked against each other.

All little endian:
  magic 76 2f 31 01; int32 version = 2 (flag bits: 0x200 tiled, 0x400 long names, 0x800 deep, 0x1000 multi-part)
  header: attributes  name\\0 type\\0 int32 size value[size]  ..., ended by one \\0
    channels (chlist): per channel name\\0, int32 type (0 UINT, 1 HALF, 2 FLOAT), uint8 pLinear, 3 x \\0, int32 xSampling, ySampling;
                       ended by \\0; channels sorted by name
    compression (1 byte: 0 NONE 1 RLE 2 ZIPS 3 ZIP 4 PIZ ...), dataWindow / displayWindow (box2i: xMin yMin xMax yMax inclusive),
    lineOrder (1 byte: 0 increasing, 1 decreasing), pixelAspectRatio float, screenWindowCenter v2f, screenWindowWidth float
  offsets: one uint64 per chunk (absolute position); chunks = ceil(height / L), L = 1 (NONE, ZIPS) or 16 (ZIP)
  chunk: int32 y of its first line, int32 dataSize, data
  raw block: per scan line, per channel in name order, that channel's values for xMin..xMax
  ZIP/ZIPS: t = even-indexed bytes of raw then odd-indexed; d[0] = t[0], d[i] = t[i] - t[i-1] + 128 (mod 256); zlib stream of d;
            a block that does not get smaller is stored raw (dataSize == raw size tells).
"""
import struct
import zlib

import numpy as np

MAGIC = b"\x76\x2f\x31\x01"
NONE, RLE, ZIPS, ZIP, PIZ = 0, 1, 2, 3, 4
UINT, HALF, FLOAT = 0, 1, 2
_DTYPE = {UINT: np.dtype("<u4"), HALF: np.dtype("<u2"), FLOAT: np.dtype("<u4")}


def lines_per_chunk(compression):
    return 16 if compression == ZIP else 1


def zip_encode(raw):
    """The chunk payload of a raw block, and whether it was stored compressed."""
    b = np.frombuffer(raw, dtype=np.uint8)
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 255
    z = zlib.compress(d.astype(np.uint8).tobytes())
    return (z, True) if len(z) < len(raw) else (bytes(raw), False)


def zip_decode(data, raw_size):
    if len(data) == raw_size:
        return bytes(data)
    d = np.frombuffer(zlib.decompress(data), dtype=np.uint8).astype(np.int64)
    assert d.size == raw_size, (d.size, raw_size)
    t = (np.cumsum(d - 128) + 128) & 255   # t[i] = t[i-1] + d[i] - 128, t[0] = d[0]
    t = t.astype(np.uint8)
    half = (raw_size + 1) // 2
    out = np.empty(raw_size, dtype=np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def _attr(name, typ, value):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def write_exr(path, planes, pixel_type=HALF, compression=ZIP, data_origin=(0, 0), display_size=None, decreasing=False,
              extra_attrs=(), version=2, channel_types=None, stored=None):
    """planes: {channel name: (h, w) array of BITS (uint16 for HALF, uint32 for FLOAT / UINT)}.
    channel_types: {name: type} to override pixel_type per channel (for files a reader must refuse).
    extra_attrs: (name, type, bytes) triples added to the header.  stored: a list that receives, per chunk, whether it was compressed.
    Returns the file's bytes (also written to `path` when it is not None)."""
    names = sorted(planes)
    h, w = planes[names[0]].shape
    types = {n: (channel_types or {}).get(n, pixel_type) for n in names}
    x0, y0 = data_origin
    fx, fy = display_size if display_size is not None else (w, h)
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", types[n], 0, 1, 1) for n in names) + b"\0"
    attrs = [
        ("channels", "chlist", chlist),
        ("compression", "compression", bytes([compression])),
        ("dataWindow", "box2i", struct.pack("<4i", x0, y0, x0 + w - 1, y0 + h - 1)),
        ("displayWindow", "box2i", struct.pack("<4i", 0, 0, fx - 1, fy - 1)),
        ("lineOrder", "lineOrder", bytes([1 if decreasing else 0])),
        ("pixelAspectRatio", "float", struct.pack("<f", 1.0)),
        ("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0)),
        ("screenWindowWidth", "float", struct.pack("<f", 1.0)),
    ] + list(extra_attrs)
    header = MAGIC + struct.pack("<i", version) + b"".join(_attr(*a) for a in sorted(attrs)) + b"\0"
    L = lines_per_chunk(compression)
    blocks = []
    for first in range(0, h, L):
        raw = b"".join(np.ascontiguousarray(planes[n][y], dtype=_DTYPE[types[n]]).tobytes()
                       for y in range(first, min(first + L, h)) for n in names)
        if compression in (ZIPS, ZIP):
            data, was = zip_encode(raw)
        else:
            data, was = raw, False
        if stored is not None:
            stored.append(was)
        blocks.append(struct.pack("<ii", y0 + first, len(data)) + data)
    order = list(range(len(blocks)))
    if decreasing:   # the chunks lie in the file bottom block first; the offset table stays in increasing y
        order.reverse()
    pos = len(header) + 8 * len(blocks)
    offsets = [0] * len(blocks)
    body = b""
    for k in order:
        offsets[k] = pos + len(body)
        body += blocks[k]
    out = header + struct.pack("<%dQ" % len(blocks), *offsets) + body
    if path is not None:
        with open(path, "wb") as f:
            f.write(out)
    return out


def _cstr(buf, pos):
    end = buf.index(b"\0", pos)
    return buf[pos:end].decode(), end + 1


def read_exr(path):
    """-> dict: planes {name: (h, w) array of bits}, types {name: type}, order (names as the file lists them), dataWindow,
    displayWindow, compression, lineOrder, attrs {name: (type, bytes)}, header_size, file_size, chunk_sizes."""
    buf = open(path, "rb").read()
    assert buf[:4] == MAGIC, "magic"
    version, = struct.unpack_from("<i", buf, 4)
    assert version & 0xff == 2 and not version & 0x1a00, version
    pos = 8
    attrs = {}
    while buf[pos] != 0:
        name, pos = _cstr(buf, pos)
        typ, pos = _cstr(buf, pos)
        size, = struct.unpack_from("<i", buf, pos)
        pos += 4
        attrs[name] = (typ, buf[pos:pos + size])
        pos += size
    pos += 1
    header_size = pos
    order, types = [], {}
    ch = attrs["channels"][1]
    p = 0
    while ch[p] != 0:
        n, p = _cstr(ch, p)
        t, _lin, xs, ys = struct.unpack_from("<iB3xii", ch, p)
        p += 16
        assert xs == 1 and ys == 1
        order.append(n)
        types[n] = t
    dw = struct.unpack("<4i", attrs["dataWindow"][1])
    disp = struct.unpack("<4i", attrs["displayWindow"][1])
    compression = attrs["compression"][1][0]
    w, h = dw[2] - dw[0] + 1, dw[3] - dw[1] + 1
    L = lines_per_chunk(compression)
    n_chunks = (h + L - 1) // L
    offsets = struct.unpack_from("<%dQ" % n_chunks, buf, pos)
    planes = {n: np.zeros((h, w), dtype=_DTYPE[types[n]]) for n in order}
    chunk_sizes = []
    for off in offsets:
        y, size = struct.unpack_from("<ii", buf, off)
        first = y - dw[1]
        lines = min(L, h - first)
        raw_size = sum(lines * w * _DTYPE[types[n]].itemsize for n in order)
        data = buf[off + 8:off + 8 + size]
        assert len(data) == size
        raw = zip_decode(data, raw_size) if compression in (ZIPS, ZIP) else data
        assert len(raw) == raw_size
        chunk_sizes.append(size)
        q = 0
        for l in range(lines):
            for n in order:
                dt = _DTYPE[types[n]]
                planes[n][first + l] = np.frombuffer(raw, dtype=dt, count=w, offset=q)
                q += w * dt.itemsize
    return dict(planes=planes, types=types, order=order, dataWindow=dw, displayWindow=disp, compression=compression,
                lineOrder=attrs["lineOrder"][1][0], attrs=attrs, header_size=header_size, file_size=len(buf), chunk_sizes=chunk_sizes)


def attr_int(info, name):
    typ, val = info["attrs"][name]
    assert typ == "int", typ
    return struct.unpack("<i", val)[0]


def attr_float(info, name):
    typ, val = info["attrs"][name]
    assert typ == "float", typ
    return struct.unpack("<f", val)[0]


def rgb_bits(info):
    """(h, w, 3) bits in R, G, B order of a file with those channels."""
    return np.stack([info["planes"][c] for c in "RGB"], axis=-1)


def half_bits(v):
    """Half(float) as the reference converts: NumPy's round-to-nearest-even float16 for every non-NaN (subnormals, >= 65520 -> inf),
    and 0x7e00 | sign for any NaN (NumPy keeps payload bits there)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16).view(np.uint16).copy()
    nan = np.isnan(v)
    sign = ((v.view(np.uint32) >> 16) & 0x8000).astype(np.uint16)
    h[nan] = 0x7e00 | sign[nan]
    return h


def write_pfm(path, img):
    """(h, w, 3) or (h, w) float32, rows top first -> PFM (bottom row first, little endian)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.000000\n" % (b"PF" if img.ndim == 3 else b"Pf", img.shape[1], img.shape[0]))
        f.write(img[::-1].astype("<f4").tobytes())


def read_pfm(path):
    """-> (h, w, 3) or (h, w) float32, rows top first."""
    buf = open(path, "rb").read()
    pos, toks = 0, []
    while len(toks) < 4:
        while buf[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not buf[end:end + 1].isspace():
            end += 1
        toks.append(buf[pos:end])
        pos = end
    pos += 1
    nc = 3 if toks[0] == b"PF" else 1
    w, h, scale = int(toks[1]), int(toks[2]), float(toks[3])
    assert scale == -1.0, scale
    a = np.frombuffer(buf, dtype="<f4", count=w * h * nc, offset=pos).reshape((h, w, 3) if nc == 3 else (h, w))
    return a[::-1].copy()
