"""vspg_pbrt --mse-reference-image / --mse-reference-out (cmd/pbrt.cpp:60-61, :244-248; cpu/integrators.cpp:129-158): the argument
and image checks, which run before --parse-only returns and need no device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
EXE = os.path.join(HOST, "vspg_pbrt")
SCENE = os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")   # film 64 x 48
W, H = 64, 48


@pytest.fixture(scope="module", autouse=True)
def host_build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc"), "libvspg_hip.so"])
    subprocess.check_call(["make", "-C", HOST])


def write_pfm(path, img):
    """RGB float32, scanlines bottom to top, little endian (util/image.cpp:1756-1800)"""
    img = np.ascontiguousarray(img, dtype="<f4")
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(img[::-1].tobytes())


def run(*args):
    return subprocess.run([EXE, SCENE, "--parse-only"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_each_option_needs_the_other(tmp_path):
    ref = tmp_path / "ref.pfm"
    write_pfm(ref, np.zeros((H, W, 3)))
    a = run("--mse-reference-image", ref)
    assert a.returncode != 0 and "--mse-reference-out" in a.stderr, a.stdout + a.stderr
    b = run("--mse-reference-out", tmp_path / "m.txt")
    assert b.returncode != 0 and "--mse-reference-image" in b.stderr, b.stdout + b.stderr
    assert not (tmp_path / "m.txt").exists()
    c = run()
    assert c.returncode == 0, c.stdout + c.stderr


def test_missing_reference_image(tmp_path):
    a = run("--mse-reference-image", tmp_path / "nothing.pfm", "--mse-reference-out", tmp_path / "m.txt")
    assert a.returncode != 0 and "nothing.pfm" in a.stderr, a.stdout + a.stderr


def test_wrong_size_names_both_sizes(tmp_path):
    ref = tmp_path / "ref.pfm"
    write_pfm(ref, np.zeros((31, 50, 3)))
    a = run("--mse-reference-image", ref, "--mse-reference-out", tmp_path / "m.txt")
    assert a.returncode != 0 and "50 x 31" in a.stderr and "64 x 48" in a.stderr, a.stdout + a.stderr
    # with pixel bounds the message names their size as well; a frame of the wrong size stays wrong
    b = run("--pixelbounds", "13,60,5,40", "--mse-reference-image", ref, "--mse-reference-out", tmp_path / "m.txt")
    assert b.returncode != 0 and "50 x 31" in b.stderr and "64 x 48" in b.stderr and "47 x 35" in b.stderr, b.stdout + b.stderr


def test_frame_sized_and_bounds_sized_images_are_accepted(tmp_path):
    frame, crop = tmp_path / "frame.pfm", tmp_path / "crop.pfm"
    write_pfm(frame, np.full((H, W, 3), 0.25))
    write_pfm(crop, np.full((35, 47, 3), 0.25))
    for ref in (frame, crop):
        a = run("--pixelbounds", "13,60,5,40", "--mse-reference-image", ref, "--mse-reference-out", tmp_path / "m.txt")
        assert a.returncode == 0, a.stdout + a.stderr
        assert "pixel bounds: [ (13, 5) - (60, 40) ]" in a.stdout and "MSE reference image" in a.stdout
    a = run("--mse-reference-image", frame, "--mse-reference-out", tmp_path / "m.txt")
    assert a.returncode == 0, a.stdout + a.stderr
    b = run("--mse-reference-image", crop, "--mse-reference-out", tmp_path / "m.txt")   # without bounds the crop is no frame
    assert b.returncode != 0 and "47 x 35" in b.stderr, b.stdout + b.stderr
