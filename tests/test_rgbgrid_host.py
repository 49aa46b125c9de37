"""RGBGridMedium ("rgbgrid") through the host adapter and scene files: CreateMedium's parameter names, defaults and error triggers and
the record the reader makes of tests/scenes/rgb_smoke.pbrt (tests/rgbgrid_host_check.cpp, two CPU tests), `--parse-only`, and on the
GPU the route: `vspg_pbrt tests/scenes/rgb_smoke.pbrt` == the same scene through the C-ABI, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
SCENE = os.path.join(ROOT, "tests", "scenes", "rgb_smoke.pbrt")
f32 = np.float32

# the grids of tests/scenes/rgb_smoke.pbrt, voxel-major with x fastest: [nz = 3, ny = 2, nx = 2, 3]
SIGMA_A = [0.125, 0.25, 0.5, 0.25, 0.125, 0, 0, 0, 0.25, 0.5, 0.5, 0.125,
           0.25, 0, 0.125, 0.125, 0.125, 0.125, 0.375, 0.25, 0, 0, 0.5, 0.25,
           0.5, 0.125, 0.25, 0, 0, 0, 0.125, 0.375, 0.5, 0.25, 0.25, 0.25]
SIGMA_S = [1, 0.5, 0.25, 2, 1.5, 1, 0.5, 2, 1.25, 0, 0, 0,
           1.5, 1.5, 0.5, 0.25, 1, 2, 1, 1, 1, 2, 0.25, 0.5,
           0.75, 0.5, 1.75, 1.25, 2, 0.25, 0, 1, 0.5, 0.5, 0.75, 1]
LE = [0, 0, 0, 1, 0.5, 0.25, 0, 0, 0, 0.25, 0.5, 1,
      2, 1, 0.5, 0, 0, 0, 0, 0.125, 0, 0.5, 0.5, 0.5,
      0, 0, 0, 0.125, 0, 0.25, 1, 1, 0, 0, 0, 0]
PLACE = [[1.5, 0, 0, 0.125], [0, 1.25, 0, -0.125], [0, 0, 1.5, 0], [0, 0, 0, 1]]   # Translate(.125, -.125, 0) * Scale(1.5, 1.25, 1.5)


@pytest.fixture(scope="module")
def host_build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc"), "libvspg_hip.so"])
    subprocess.check_call(["make", "-C", HOST])
    return HOST


@pytest.fixture(scope="module")
def host_check(host_build, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rgbgrid_host") / "rgbgrid_host_check")
    csrc = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "rgbgrid_host_check.cpp"),
                           "-L" + HOST, "-lvspg_host", "-L" + csrc, "-lvspg_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + csrc])
    return lambda arg: subprocess.run([exe, arg], capture_output=True, text=True, timeout=120)


def test_create_medium_parameters_and_errors(host_check):
    """The adapter's CreateMedium("rgbgrid"): names, defaults, storage, and every error trigger of media.cpp:418-445 by its words."""
    p = host_check("create")
    print(p.stdout)
    assert p.returncode == 0 and "all checks passed" in p.stdout, p.stdout + p.stderr


def test_scene_file_parses_into_the_expected_record(host_check, host_build):
    """MakeNamedMedium "string type" "rgbgrid" under a CTM: type, size, bounds, scales, the three grids in voxel order, renderFromMedium
    (checked field by field in tests/rgbgrid_host_check.cpp); and what `vspg_pbrt --parse-only` reports."""
    p = host_check(SCENE)
    print(p.stdout)
    assert p.returncode == 0 and "all checks passed" in p.stdout, p.stdout + p.stderr
    a = subprocess.run([os.path.join(host_build, "vspg_pbrt"), SCENE, "--parse-only"], capture_output=True, text=True)
    assert a.returncode == 0, a.stdout + a.stderr
    assert "medium type 4 (placed)" in a.stdout and "film 24x16 @ 4 spp" in a.stdout, a.stdout
    assert "RGB grid 2 x 2 x 3: sigma_a sigma_s Le, scale 2, Lescale 0.5" in a.stdout, a.stdout
    assert len(SIGMA_A) == len(SIGMA_S) == len(LE) == 36 and (sum(SIGMA_A), sum(SIGMA_S), sum(LE)) == (7.375, 32.75, 11.0)   # the sums the C++ check pins


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1]


@pytest.mark.gpu
def test_scene_file_render_equals_the_api_scene(host_build, gpu_pkg, tmp_path):
    """`vspg_pbrt tests/scenes/rgb_smoke.pbrt` == the same scene through the C-ABI (the fog box, set_rgb_grid_medium,
    set_medium_transform, "nds"), bit for bit; the Le grid matters under "nds": without it the film differs."""
    exe = os.path.join(host_build, "vspg_pbrt")
    out = tmp_path / "smoke.pfm"
    a = subprocess.run([exe, SCENE, "--outfile", str(out)], capture_output=True, text=True)
    assert a.returncode == 0, a.stdout + a.stderr
    P = gpu_pkg
    W, H, spp = 24, 16, 4
    grid = lambda v: np.array(v, dtype=f32).reshape(3, 2, 2, 3)

    def render(le):
        s = P.fog_box_scene(W, H)
        P.set_rgb_grid_medium(s, grid(SIGMA_A), grid(SIGMA_S), le, p0=(-0.5,) * 3, p1=(0.5,) * 3, g=0.25, scale=2.0, Lescale=0.5)
        P.set_medium_transform(s, PLACE)
        prm = P.app_f_params()
        prm.vspsamplingmethod = P.VSP_NDS
        r = P.Renderer(s, prm, W, H)
        assert r.kernel_name() == "k_wf_segment_vertex<RgbGridMedium>"
        for w in range(spp):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        f = r.film()
        r.close()
        return (f[..., :3] / f[..., 3:4]).astype(np.float32)

    img = read_pfm(str(out))
    assert np.isfinite(img).all() and img.max() > 0
    assert np.array_equal(img.view(np.uint32), render(grid(LE)).view(np.uint32))
    assert not np.array_equal(img.view(np.uint32), render(None).view(np.uint32))
