"""The host's image layer (host/vspg_image.h: PFM and the OpenEXR subset) against the test-side model tests/exr_model.py, through
the no-device tool host/vspg_imgtool.  Every comparison is of bits or bytes.

VSPG_IMGTOOL in the environment names another build of the tool (scripts/run_sanitized_cpu_tests.sh: the ASan + UBSan one)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import exr_model as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")

SIZES = [(7, 5), (37, 19)]       # (w, h): one ZIP block, and two of which the second is short
ORIGIN, DISPLAY = (3, 2), (64, 48)
COMPRESSIONS = [(X.NONE, "none"), (X.ZIPS, "zips"), (X.ZIP, "zip")]


@pytest.fixture(scope="module")
def tool():
    if os.environ.get("VSPG_IMGTOOL"):
        return os.environ["VSPG_IMGTOOL"]
    subprocess.check_call(["make", "-C", HOST, "vspg_imgtool"])
    return os.path.join(HOST, "vspg_imgtool")


def run(tool, *args):
    return subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)


def ok(tool, *args):
    r = run(tool, *args)
    assert r.returncode == 0, r.stderr
    return r


def smooth_image(w, h):
    """float32 (h, w, 3): a ramp, exactly representable in half, that ZIP shrinks."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 0.25, y * 0.5, (x + y) * 0.125 - 1.0], axis=-1).astype(np.float32)


def random_bits(w, h, pixel_type, seed):
    """(h, w, 3) random bit patterns with random mantissas -- incompressible -- and no NaN or inf exponent (widening a signalling NaN
    is not a bit-exact operation on every CPU NumPy runs on; the NaN rules have a test of their own)."""
    rng = np.random.default_rng(seed)
    if pixel_type == X.HALF:
        b = rng.integers(0, 1 << 16, size=(h, w, 3), dtype=np.uint32).astype(np.uint16)
        b[(b & 0x7c00) == 0x7c00] &= 0xbfff
        return b
    b = rng.integers(0, 1 << 32, size=(h, w, 3), dtype=np.uint64).astype(np.uint32)
    b[(b & 0x7f800000) == 0x7f800000] &= 0xbfffffff
    return b


def bits_of(img, pixel_type):
    """float32 image -> the bits of its HALF or FLOAT samples."""
    return X.half_bits(img) if pixel_type == X.HALF else np.ascontiguousarray(img, dtype=np.float32).view(np.uint32)


def as_float(bits, pixel_type):
    return bits.view(np.float16).astype(np.float32) if pixel_type == X.HALF else bits.view(np.float32)


def planes_of(bits):
    return {c: bits[..., i] for i, c in enumerate("RGB")}


@pytest.mark.parametrize("decreasing", [False, True], ids=["incy", "decy"])
@pytest.mark.parametrize("compression,cname", COMPRESSIONS, ids=[c[1] for c in COMPRESSIONS])
@pytest.mark.parametrize("pixel_type", [X.HALF, X.FLOAT], ids=["half", "float"])
@pytest.mark.parametrize("w,h", SIZES)
def test_model_exr_to_pfm(tool, tmp_path, w, h, pixel_type, compression, cname, decreasing):
    bits = bits_of(smooth_image(w, h), pixel_type)
    X.write_exr(tmp_path / "a.exr", planes_of(bits), pixel_type, compression, ORIGIN, DISPLAY, decreasing)
    ok(tool, "convert", tmp_path / "a.exr", tmp_path / "a.pfm")
    got = X.read_pfm(tmp_path / "a.pfm")
    assert np.array_equal(got.view(np.uint32), as_float(bits, pixel_type).view(np.uint32))
    info = json.loads(ok(tool, "info", tmp_path / "a.exr").stdout)
    assert info["dataWindow"] == [3, 2, 3 + w - 1, 2 + h - 1] and info["displayWindow"] == [0, 0, 63, 47]
    assert info["channels"] == ["B", "G", "R"] and info["type"] == ("half" if pixel_type == X.HALF else "float")
    assert info["compression"] == compression and info["lineOrder"] == int(decreasing)


@pytest.mark.parametrize("pixel_type", [X.HALF, X.FLOAT], ids=["half", "float"])
@pytest.mark.parametrize("w,h", SIZES)
def test_zip_block_stored_raw(tool, tmp_path, w, h, pixel_type):
    """Random mantissas do not compress: the ZIP chunk holds the raw block, which a reader tells by its size alone."""
    bits = random_bits(w, h, pixel_type, 5)
    stored = []
    X.write_exr(tmp_path / "r.exr", planes_of(bits), pixel_type, X.ZIP, ORIGIN, DISPLAY, stored=stored)
    assert not all(stored), "the test image was meant to hold a block that does not compress"
    ok(tool, "convert", tmp_path / "r.exr", tmp_path / "r.pfm")
    assert np.array_equal(X.read_pfm(tmp_path / "r.pfm").view(np.uint32), as_float(bits, pixel_type).view(np.uint32))
    # and the writer does the same: its file reads back, with at least one chunk of exactly the raw size
    ok(tool, "convert", tmp_path / "r.exr", tmp_path / "r2.exr", "--compression", "zip")
    info = X.read_exr(tmp_path / "r2.exr")
    assert np.array_equal(X.rgb_bits(info), bits)
    bps = 2 if pixel_type == X.HALF else 4
    assert info["chunk_sizes"][0] == min(16, h) * w * 3 * bps


def test_unknown_attribute_is_skipped(tool, tmp_path):
    w, h = 7, 5
    bits = bits_of(smooth_image(w, h), X.FLOAT)
    extra = [("zzComment", "string", b"written by a tool this reader has never heard of"), ("aaBox", "box2f", struct.pack("<4f", 0, 0, 1, 1)),
             ("samplesPerPixel", "int", struct.pack("<i", 12)), ("MSE", "float", struct.pack("<f", 0.125))]
    X.write_exr(tmp_path / "e.exr", planes_of(bits), X.FLOAT, X.ZIP, ORIGIN, DISPLAY, extra_attrs=extra, version=2 | 0x400)
    ok(tool, "convert", tmp_path / "e.exr", tmp_path / "e.pfm")
    assert np.array_equal(X.read_pfm(tmp_path / "e.pfm").view(np.uint32), bits)
    info = json.loads(ok(tool, "info", tmp_path / "e.exr").stdout)
    assert info["samplesPerPixel"] == 12 and info["MSE"] == 0.125


@pytest.mark.parametrize("compression,cname", COMPRESSIONS, ids=[c[1] for c in COMPRESSIONS])
@pytest.mark.parametrize("pixel_type,flag", [(X.HALF, "--fp16"), (X.FLOAT, "--fp32")], ids=["half", "float"])
@pytest.mark.parametrize("w,h", SIZES)
def test_pfm_to_exr(tool, tmp_path, w, h, pixel_type, flag, compression, cname):
    img = smooth_image(w, h) + np.float32(1.0 / 3.0)   # (not representable in half: the conversion rounds)
    X.write_pfm(tmp_path / "a.pfm", img)
    ok(tool, "convert", tmp_path / "a.pfm", tmp_path / "a.exr", flag, "--compression", cname)
    info = X.read_exr(tmp_path / "a.exr")
    assert info["order"] == ["B", "G", "R"]
    assert all(t == pixel_type for t in info["types"].values())
    assert np.array_equal(X.rgb_bits(info), bits_of(img, pixel_type))
    assert info["dataWindow"] == (0, 0, w - 1, h - 1) and info["displayWindow"] == (0, 0, w - 1, h - 1)
    assert info["compression"] == compression and info["lineOrder"] == 0
    bps = 2 if pixel_type == X.HALF else 4
    # the eight required attributes and nothing else: 313 bytes for three channels with one-letter names
    assert info["header_size"] == 313
    assert sorted(info["attrs"]) == ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio",
                                     "screenWindowCenter", "screenWindowWidth"]
    if compression == X.NONE:
        assert info["file_size"] == 313 + 8 * h + h * (8 + 3 * w * bps)
        if (w, h, pixel_type) == (7, 5, X.HALF):
            assert info["file_size"] == 603
    # the model's own file of the same image is the same file when nothing is compressed (zlib versions may differ otherwise)
    if compression == X.NONE:
        want = X.write_exr(None, planes_of(bits_of(img, pixel_type)), pixel_type, X.NONE)
        assert open(tmp_path / "a.exr", "rb").read() == want


@pytest.mark.parametrize("compression,cname", COMPRESSIONS, ids=[c[1] for c in COMPRESSIONS])
def test_exr_to_exr_keeps_windows_and_metadata(tool, tmp_path, compression, cname):
    w, h = 37, 19
    bits = bits_of(smooth_image(w, h), X.HALF)
    extra = [("samplesPerPixel", "int", struct.pack("<i", 3)), ("renderTimeSeconds", "float", struct.pack("<f", 1.5))]
    X.write_exr(tmp_path / "a.exr", planes_of(bits), X.HALF, X.ZIPS, ORIGIN, DISPLAY, decreasing=True, extra_attrs=extra)
    ok(tool, "convert", tmp_path / "a.exr", tmp_path / "b.exr", "--compression", cname)
    info = X.read_exr(tmp_path / "b.exr")
    assert info["dataWindow"] == (3, 2, 3 + w - 1, 2 + h - 1) and info["displayWindow"] == (0, 0, 63, 47)
    assert info["compression"] == compression and info["lineOrder"] == 0
    assert np.array_equal(X.rgb_bits(info), bits)
    assert X.attr_int(info, "samplesPerPixel") == 3 and X.attr_float(info, "renderTimeSeconds") == 1.5


def edge_values():
    """The values at which Half(float) can go wrong."""
    f = np.float32
    bits = [0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffa5a5a5]   # NaNs: quiet, signalling, both signs, payloads
    vals = [0.0, -0.0, 6e-8, 5.9604645e-8, 2.9802322e-8, 2.9802326e-8, 2.98e-8, 8.9406967e-8, 6e-5, 6.1035156e-5, 6.0975552e-5, 6.1e-5, 1e-10, -1e-10,
            1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 2047.5, 2048.5, 2049.0, 2051.0,   # exact ties, both parities
            65504.0, 65505.0, 65519.996, 65520.0, 65536.0, 1e9, np.inf, -65504.0, -65519.996, -65520.0, -70000.0, -np.inf, 0.1, -0.3, 1 / 3]
    v = np.concatenate([np.array(bits, dtype=np.uint32).view(np.float32), np.array(vals, dtype=f)])
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([v, -v, rnd])


def test_half_conversion_on_the_host(tool, tmp_path):
    v = edge_values()
    w = 61
    h = -(-v.size // (3 * w))
    img = np.zeros(h * w * 3, dtype=np.float32)
    img[:v.size] = v
    img = img.reshape(h, w, 3)
    X.write_pfm(tmp_path / "edge.pfm", img)
    assert np.array_equal(X.read_pfm(tmp_path / "edge.pfm").view(np.uint32), img.view(np.uint32))
    ok(tool, "convert", tmp_path / "edge.pfm", tmp_path / "edge.exr", "--fp16", "--compression", "zip")
    info = X.read_exr(tmp_path / "edge.exr")
    want = X.half_bits(img)
    got = X.rgb_bits(info)
    assert np.array_equal(got, want), [(hex(a), hex(b), hex(c)) for a, b, c in zip(img.view(np.uint32)[got != want], got[got != want], want[got != want])][:8]
    nan = np.isnan(img)
    assert nan.sum() >= 12 and set(np.unique(got[nan])) == {0x7e00, 0xfe00}


def _refused(tool, path, *words):
    r = run(tool, "info", path)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)   # (a crash or a sanitizer report is another code)
    assert r.stderr.startswith("error: ") and os.path.basename(str(path)) in r.stderr, r.stderr
    for wd in words:
        assert wd in r.stderr, (wd, r.stderr)


@pytest.fixture(scope="module")
def good_file():
    bits = bits_of(smooth_image(37, 19), X.HALF)
    return X.write_exr(None, planes_of(bits), X.HALF, X.ZIP, ORIGIN, DISPLAY), bits


@pytest.mark.parametrize("where", ["header", "offsets", "chunk-header", "chunk-data", "magic"])
def test_truncated_files_are_refused(tool, tmp_path, good_file, where):
    data, _ = good_file
    header = data.index(b"screenWindowWidth") + 18 + 6 + 4 + 4 + 1
    first_chunk, = struct.unpack_from("<Q", data, header)
    cut = {"header": data.index(b"dataWindow") + 14, "offsets": header + 11, "chunk-header": first_chunk + 5, "chunk-data": len(data) - 9, "magic": 3}[where]
    p = tmp_path / ("cut_%s.exr" % where)
    p.write_bytes(data[:cut])
    _refused(tool, p, "truncated" if where not in ("chunk-header", "chunk-data") else "")
    if where == "chunk-data":
        _refused(tool, p, "past the end of the file")
    if where == "chunk-header":
        _refused(tool, p, "outside the file")


def test_wild_offsets_and_sizes_are_refused(tool, tmp_path, good_file):
    data, _ = good_file
    header = data.index(b"screenWindowWidth") + 18 + 6 + 4 + 4 + 1
    for k, off in enumerate([len(data) + 100, len(data) - 4, 2 ** 63, 2 ** 64 - 1]):
        p = tmp_path / ("off%d.exr" % k)
        p.write_bytes(data[:header + 8] + struct.pack("<Q", off) + data[header + 16:])
        _refused(tool, p, "outside the file")
    first, = struct.unpack_from("<Q", data, header)
    for k, size in enumerate([0x7fffffff, -5, len(data)]):
        p = tmp_path / ("size%d.exr" % k)
        p.write_bytes(data[:first + 4] + struct.pack("<i", size) + data[first + 8:])
        _refused(tool, p, "chunk 0")
    # a chunk that claims a scan line outside the data window, and one that is there twice
    p = tmp_path / "line.exr"
    p.write_bytes(data[:first] + struct.pack("<i", 1000) + data[first + 4:])
    _refused(tool, p, "scan line 1000")
    p = tmp_path / "twice.exr"
    p.write_bytes(data[:header + 8] + struct.pack("<Q", first) + data[header + 16:])
    _refused(tool, p, "two chunks")
    # a compressed block whose bytes are not a zlib stream
    p = tmp_path / "garbage.exr"
    p.write_bytes(data[:first + 8] + bytes(16) + data[first + 24:])
    _refused(tool, p, "inflate")
    # a data window larger than anything the file could hold
    at = data.index(b"dataWindow\0box2i\0") + 17 + 4
    p = tmp_path / "huge.exr"
    p.write_bytes(data[:at] + struct.pack("<4i", 0, 0, 2 ** 31 - 2, 2 ** 31 - 2) + data[at + 16:])
    _refused(tool, p, "data window")


def test_unsupported_files_are_refused_by_name(tool, tmp_path, good_file):
    _, bits = good_file
    planes = planes_of(bits)
    for flag, word in [(0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")]:
        p = tmp_path / ("flag%x.exr" % flag)
        X.write_exr(p, planes, X.HALF, X.ZIP, version=2 | flag)
        _refused(tool, p, word)
    for comp, word in [(X.PIZ, "PIZ"), (X.RLE, "RLE"), (8, "DWAA")]:
        p = tmp_path / ("comp%d.exr" % comp)
        X.write_exr(p, planes, X.HALF, comp)
        _refused(tool, p, word, "compression")
    p = tmp_path / "uint.exr"
    X.write_exr(p, {c: v.astype(np.uint32) for c, v in planes.items()}, X.UINT, X.NONE)
    _refused(tool, p, "UINT")
    p = tmp_path / "mixed.exr"
    X.write_exr(p, {"B": planes["B"], "G": planes["G"].astype(np.uint32), "R": planes["R"]}, X.HALF, X.NONE, channel_types={"G": X.FLOAT})
    _refused(tool, p, "mixed channel types")
    p = tmp_path / "notexr.exr"
    p.write_bytes(b"PF\n1 1\n-1.0\n" + bytes(12))
    _refused(tool, p, "magic")
    r = run(tool, "info", tmp_path / "absent.exr")
    assert r.returncode == 1 and "cannot open" in r.stderr
    r = run(tool, "info", tmp_path / "image.png")
    assert r.returncode == 1 and "extension" in r.stderr


def test_channel_list_that_runs_past_its_attribute_is_refused(tool, tmp_path, good_file):
    """The channel list is bounded by its attribute's size, not by the file's: a name, the reserved bytes or the sampling fields that
    run past it are refused before anything behind them is read."""
    head = X.MAGIC + struct.pack("<i", 2) + b"channels\0chlist\0"
    cases = {
        "name_past_size_at_eof": head + struct.pack("<i", 1) + b"A" + b"B\0" + bytes(4),           # 35 bytes: the name runs out of the attribute, the file ends in the fields
        "name_past_size": head + struct.pack("<i", 1) + b"A" + b"B\0" + bytes(64),
        "fields_past_size": head + struct.pack("<i", 8) + b"R\0" + struct.pack("<iB3xii", 1, 0, 1, 1) + b"\0" + bytes(64),
        "no_terminator": head + struct.pack("<i", 18) + b"R\0" + struct.pack("<iB3xii", 1, 0, 1, 1) + b"G" * 40,
        "size_zero": head + struct.pack("<i", 0) + b"\0" + bytes(64),
    }
    for name, data in cases.items():
        p = tmp_path / (name + ".exr")
        p.write_bytes(data)
        _refused(tool, p, "channel list runs past its attribute's size")
    # the same inside an otherwise good file: the attribute's size cut to the middle of the second channel
    data, _ = good_file
    at = data.index(b"channels\0chlist\0") + 16
    size, = struct.unpack_from("<i", data, at)
    assert size == 55
    p = tmp_path / "short_size.exr"
    p.write_bytes(data[:at] + struct.pack("<i", 25) + data[at + 4:])
    _refused(tool, p, "channel list runs past its attribute's size")


@pytest.mark.parametrize("compression", [X.NONE, X.ZIPS, X.ZIP], ids=["none", "zips", "zip"])
def test_data_window_larger_than_the_file_could_hold_is_refused(tool, tmp_path, compression):
    """A file of a few KB whose data window asks for gigabytes of pixels is refused from its header and offset table alone."""
    w, h = 7, 5
    bits = bits_of(smooth_image(w, h), X.FLOAT)
    data = X.write_exr(None, planes_of(bits), X.FLOAT, compression)
    at = data.index(b"dataWindow\0box2i\0") + 17 + 4
    # 32768 wide (the reader's own limit) and as many rows as the file still has an offset table for
    rows = 4 if compression != X.ZIP else 64
    big = data[:at] + struct.pack("<4i", 0, 0, 32767, rows - 1) + data[at + 16:]
    p = tmp_path / "big.exr"
    p.write_bytes(big + bytes(8 * rows))
    _refused(tool, p, "bytes of pixels")
