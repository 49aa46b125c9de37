"""The host adapter's frame loop over a volume sequence: example_render's "sequence" mode renders two frames of
a 12^3 "uniformgrid" medium through ONE integrator -- SetMediumDensity, ClearFilm, Render -- and both frames equal the same calls
driven through the raw C-ABI, bit for bit; a density of the wrong size and a temperature grid the scene never had are refused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import grid_scene

HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc"), "libvspg_hip.so"])
    subprocess.check_call(["make", "-C", HOST])
    return HOST


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        data = np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)
    return data[::-1]


def frame_density(a, b, c, m):
    n = 12
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.ascontiguousarray((((i * a + j * b + k * c) % m) / np.float32(m - 1)).astype(np.float32).transpose(2, 1, 0)).ravel()  # x fastest


@pytest.mark.gpu
def test_sequence_through_the_adapter_equals_the_cabi(host_build, gpu_pkg, tmp_path):
    P = gpu_pkg
    W, H, spp = 48, 32, 3
    f0, f1 = tmp_path / "frame0.pfm", tmp_path / "frame1.pfm"
    res = subprocess.run([os.path.join(host_build, "example_render"), str(W), str(H), str(spp), str(f0), "sequence", str(f1)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    refused = [line for line in res.stdout.splitlines() if line.startswith("refused: ")]
    assert len(refused) == 2 and "n_floats" in refused[0] and "temperature" in refused[1], res.stdout
    d0, d1 = frame_density(7, 13, 29, 17), frame_density(5, 11, 3, 13)
    scene = grid_scene(d0, (12, 12, 12), (.02, .03, .04), (.5, .45, .4), g=0.3, bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=W, H=H)
    r = P.Renderer(scene, P.app_f_params(), W, H)
    frames = []
    for d in (None, d1):
        if d is not None:
            r.update_density(d)
            r.film_clear()
        for w in range(spp):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        f = r.film()
        frames.append((f[..., :3] / f[..., 3:4]).astype(np.float32))
    r.close()
    assert not np.array_equal(frames[0], frames[1]) and frames[1].max() > 0
    assert np.array_equal(read_pfm(str(f0)).view(np.uint32), frames[0].view(np.uint32))
    assert np.array_equal(read_pfm(str(f1)).view(np.uint32), frames[1].view(np.uint32))
