"""OpenEXR through the host adapter and vspg_pbrt: the film written as .exr (resolved on the device), an .exr MSE reference image,
--write-partial-images and the NDS+ transmittance buffer as .exr -- each against the same run through PFM, read with the test-side
codec tests/exr_model.py.  Bits and bytes only."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exr_model as X  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
SCENE = os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")      # 64 x 48, 4 spp
SPP = 3


@pytest.fixture(scope="module")
def exe(gpu_pkg):
    subprocess.check_call(["make", "-C", HOST])
    return os.path.join(HOST, "vspg_pbrt")


def pbrt(exe, scene, *args):
    r = subprocess.run([exe, str(scene), "--spp", str(SPP), "--seed", "5"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pfm_run(exe, tmp_path_factory):
    """The film of the reference run, through PFM: shared by the tests below."""
    d = tmp_path_factory.mktemp("pfm")
    pbrt(exe, SCENE, "--outfile", d / "a.pfm")
    img = X.read_pfm(d / "a.pfm")
    assert img.shape == (48, 64, 3) and np.isfinite(img).all() and img.max() < 65504 and img.max() > 0
    return img


def test_outfile_exr_is_half_of_the_pfm_pixels(exe, pfm_run, tmp_path):
    pbrt(exe, SCENE, "--outfile", tmp_path / "a.exr")
    info = X.read_exr(tmp_path / "a.exr")
    assert info["order"] == ["B", "G", "R"] and set(info["types"].values()) == {X.HALF}
    assert info["compression"] == X.ZIP and info["lineOrder"] == 0
    assert info["dataWindow"] == (0, 0, 63, 47) and info["displayWindow"] == (0, 0, 63, 47)
    assert np.array_equal(X.rgb_bits(info), X.half_bits(pfm_run))
    assert X.attr_int(info, "samplesPerPixel") == SPP
    assert X.attr_float(info, "renderTimeSeconds") > 0
    assert "MSE" not in info["attrs"]
    # the Film's own file name does the same as --outfile
    text = open(SCENE).read().replace('"string filename" "fog_box.pfm"', '"string filename" "%s"' % (tmp_path / "named.exr"))
    (tmp_path / "named.pbrt").write_text(text)
    pbrt(exe, tmp_path / "named.pbrt")
    assert np.array_equal(X.rgb_bits(X.read_exr(tmp_path / "named.exr")), X.half_bits(pfm_run))


def test_pixel_bounds_become_the_data_window(exe, tmp_path):
    pbrt(exe, SCENE, "--outfile", tmp_path / "b.pfm", "--pixelbounds", "13,60,5,40")
    pbrt(exe, SCENE, "--outfile", tmp_path / "b.exr", "--pixelbounds", "13,60,5,40")
    img = X.read_pfm(tmp_path / "b.pfm")
    info = X.read_exr(tmp_path / "b.exr")
    assert img.shape == (35, 47, 3)
    assert info["dataWindow"] == (13, 5, 59, 39) and info["displayWindow"] == (0, 0, 63, 47)
    assert np.array_equal(X.rgb_bits(info), X.half_bits(img))


def test_savefp16_false_gives_float_equal_to_the_pfm(exe, pfm_run, tmp_path):
    text = open(SCENE).read().replace('"string filename" "fog_box.pfm"', '"string filename" "fog_box.pfm" "bool savefp16" false')
    assert "savefp16" in text
    (tmp_path / "f32.pbrt").write_text(text)
    pbrt(exe, tmp_path / "f32.pbrt", "--outfile", tmp_path / "c.exr")
    info = X.read_exr(tmp_path / "c.exr")
    assert set(info["types"].values()) == {X.FLOAT} and info["order"] == ["B", "G", "R"]
    assert np.array_equal(X.rgb_bits(info), u32(pfm_run))
    # the parameter is accepted for a PFM film too (and changes nothing there)
    pbrt(exe, tmp_path / "f32.pbrt", "--outfile", tmp_path / "c.pfm")
    assert np.array_equal(u32(X.read_pfm(tmp_path / "c.pfm")), u32(pfm_run))


def test_mse_reference_image_as_exr(exe, pfm_run, tmp_path):
    ref = (pfm_run * np.float32(1.125) + np.float32(0.01)).astype(np.float32)     # (not the film itself: the errors are not zero)
    X.write_pfm(tmp_path / "ref.pfm", ref)
    X.write_exr(tmp_path / "ref.exr", {c: u32(ref[..., i]) for i, c in enumerate("RGB")}, X.FLOAT, X.ZIP)
    pbrt(exe, SCENE, "--outfile", tmp_path / "m1.pfm", "--mse-reference-image", tmp_path / "ref.pfm", "--mse-reference-out", tmp_path / "mse_pfm.txt")
    pbrt(exe, SCENE, "--outfile", tmp_path / "m2.exr", "--mse-reference-image", tmp_path / "ref.exr", "--mse-reference-out", tmp_path / "mse_exr.txt")
    a, b = (tmp_path / "mse_pfm.txt").read_bytes(), (tmp_path / "mse_exr.txt").read_bytes()
    assert a == b and len(a.splitlines()) == SPP
    # the written film carries the last line's value
    info = X.read_exr(tmp_path / "m2.exr")
    last = np.float32(float(a.splitlines()[-1].split(b", ")[1]))
    assert np.float32(X.attr_float(info, "MSE")) == last and last > 0
    # a half reference image is widened exactly: the same lines as its float copy
    half = X.half_bits(ref)
    X.write_exr(tmp_path / "refh.exr", {c: half[..., i] for i, c in enumerate("RGB")}, X.HALF, X.ZIPS, decreasing=True)
    X.write_pfm(tmp_path / "refh.pfm", half.view(np.float16).astype(np.float32))
    pbrt(exe, SCENE, "--outfile", tmp_path / "m3.pfm", "--mse-reference-image", tmp_path / "refh.pfm", "--mse-reference-out", tmp_path / "h_pfm.txt")
    pbrt(exe, SCENE, "--outfile", tmp_path / "m4.pfm", "--mse-reference-image", tmp_path / "refh.exr", "--mse-reference-out", tmp_path / "h_exr.txt")
    assert (tmp_path / "h_pfm.txt").read_bytes() == (tmp_path / "h_exr.txt").read_bytes() != a
    # the size rule and its words are unchanged
    X.write_exr(tmp_path / "small.exr", {c: u32(ref[:10, :20, i]) for i, c in enumerate("RGB")}, X.FLOAT, X.ZIP)
    r = subprocess.run([exe, SCENE, "--mse-reference-image", str(tmp_path / "small.exr"), "--mse-reference-out", str(tmp_path / "x.txt"), "--parse-only"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "the MSE reference image is 20 x 10" in r.stderr and "(64 x 48)" in r.stderr


def test_write_partial_images(exe, pfm_run, tmp_path):
    pbrt(exe, SCENE, "--outfile", tmp_path / "p.exr", "--write-partial-images")
    info = X.read_exr(tmp_path / "p.exr")
    assert np.array_equal(X.rgb_bits(info), X.half_bits(pfm_run)) and X.attr_int(info, "samplesPerPixel") == SPP
    pbrt(exe, SCENE, "--outfile", tmp_path / "p.pfm", "--write-partial-images")
    assert np.array_equal(u32(X.read_pfm(tmp_path / "p.pfm")), u32(pfm_run))
    # the file after the first wave: a run that --spp 1 stops there
    r = subprocess.run([exe, SCENE, "--spp", "1", "--seed", "5", "--outfile", str(tmp_path / "p1.exr"), "--write-partial-images"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, SCENE, "--spp", "1", "--seed", "5", "--outfile", str(tmp_path / "q1.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    one = X.read_exr(tmp_path / "p1.exr")
    assert X.attr_int(one, "samplesPerPixel") == 1
    assert np.array_equal(X.rgb_bits(one), X.half_bits(X.read_pfm(tmp_path / "q1.pfm")))


GRID = ('MakeNamedMedium "fog" "string type" "uniformgrid" "integer nx" 3 "integer ny" 3 "integer nz" 3 "point3 p0" [ -0.8 -0.8 -0.5 ] "point3 p1" [ 0.8 0.7 0.9 ]\n'
        '    "float density" [ 0.2 1 0.7  0.1 0.9 0.4  1 0.6 0.3    0.5 1.2 0.8  0.9 1.3 0.6  0.2 0.7 0.4    0 0.4 0.1  0.3 0.8 0.2  0.1 0.3 0 ]\n'
        '    "rgb sigma_a" [ .02 .03 .04 ] "rgb sigma_s" [ .5 .45 .4 ] "float g" 0.3\n')


def nds_scene(path, extra):
    """fog_box.pbrt with a grid medium in the box (the NDS+ workflow is a grid medium's) and the transmittance-buffer options"""
    lines = open(SCENE).read().splitlines(keepends=True)
    out = []
    for ln in lines:
        if ln.startswith("MakeNamedMedium"):
            out.append(GRID)
        elif ln.startswith("Integrator"):
            out.append(ln.rstrip("\n") + " " + extra + "\n")
        else:
            out.append(ln)
    text = "".join(out)
    assert "uniformgrid" in text and extra in text
    path.write_text(text)
    return path


def test_tr_buffer_round_trip_through_exr(exe, tmp_path):
    store = '"string vspsamplingmethod" "resampling" "bool storeTrBuffer" true "string trBufferFileName" "%s"'
    load = '"string vspsamplingmethod" "nds" "bool collisionProbabilityBias" true "bool loadTrBuffer" true "string trBufferFileName" "%s"'
    pbrt(exe, nds_scene(tmp_path / "s_pfm.pbrt", store % (tmp_path / "t.pfm")), "--outfile", tmp_path / "s1.pfm")
    pbrt(exe, nds_scene(tmp_path / "s_exr.pbrt", store % (tmp_path / "t.exr")), "--outfile", tmp_path / "s2.pfm")
    tr = X.read_pfm(tmp_path / "t.pfm")
    info = X.read_exr(tmp_path / "t.exr")
    assert info["order"] == ["Transmittance.B", "Transmittance.G", "Transmittance.R"] and set(info["types"].values()) == {X.FLOAT}
    assert info["dataWindow"] == (0, 0, 63, 47)
    got = np.stack([info["planes"]["Transmittance." + c] for c in "RGB"], axis=-1)
    assert np.array_equal(got, u32(tr)) and 0.05 < float(tr.mean()) < 0.99 and float(tr.std()) > 0
    pbrt(exe, nds_scene(tmp_path / "l_pfm.pbrt", load % (tmp_path / "t.pfm")), "--outfile", tmp_path / "l1.pfm")
    pbrt(exe, nds_scene(tmp_path / "l_exr.pbrt", load % (tmp_path / "t.exr")), "--outfile", tmp_path / "l2.pfm")
    a, b = X.read_pfm(tmp_path / "l1.pfm"), X.read_pfm(tmp_path / "l2.pfm")
    assert np.array_equal(u32(a), u32(b))
    assert not np.array_equal(u32(a), u32(X.read_pfm(tmp_path / "s1.pfm")))      # (the second pass is another estimator: it did render)
    # an .exr without the channels is refused by name
    X.write_exr(tmp_path / "rgb.exr", {c: u32(tr[..., i]) for i, c in enumerate("RGB")}, X.FLOAT, X.ZIP)
    r = subprocess.run([exe, str(nds_scene(tmp_path / "bad.pbrt", load % (tmp_path / "rgb.exr"))), "--spp", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Transmittance.R" in r.stderr
