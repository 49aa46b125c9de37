"""The image infinite light on the device: vspg_envlight_batch against the float32 mirror of tests/envlight_model.py bit for bit, the
light through whole paths (kernel families against each other, a known answer, NEE against escaping rays only), and
vspg_renderer_set_environment_image on a live renderer.  Images are seeded: 'peaked' (one texel 1e3 times the rest), 'banded' (the same
with zero rows), 'equal'."""
import math
import os

import numpy as np
import pytest

import envlight_model as M
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 48, 32
N = 4096


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rotation(scale=(1, 1, 1)):
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(0.7) * K + (1 - math.cos(0.7)) * K @ K
    m = np.zeros((3, 4), f32)
    m[:, :3] = (R @ np.diag(scale)).astype(f32)
    return m


XFORMS = {"identity": None, "rotation": rotation(), "rotation_scale": rotation((2.0, 1.25, 3.0))}
SKY_L = (0.5, 0.75, 1.25)


def sky_only_scene(P, w=8, h=8, L=SKY_L):
    """No geometry, no medium: camera and one image infinite light."""
    s = scenes.empty_scene(w, h, eye=(0, 0.2, -3), look=(0, 0, 0))
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, L)
    return s


def with_kernel(kernel, fn):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        return fn()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


@pytest.fixture(scope="module")
def batch_renderer(gpu_pkg):
    r = gpu_pkg.Renderer(sky_only_scene(gpu_pkg), gpu_pkg.app_f_params(), 8, 8)
    yield r
    r.close()


COLS = {"Le": slice(0, 3), "Le uv": slice(3, 5), "PDF_Li": slice(5, 6), "SampleLi valid": slice(6, 7), "SampleLi uv": slice(7, 9),
        "SampleLi wi": slice(9, 12), "SampleLi pdf": slice(12, 13), "SampleLi L": slice(13, 16)}


def assert_batch_equals_mirror(got, want, what):
    for name, c in COLS.items():
        bad = np.argwhere(u32(got[:, c]) != u32(want[:, c]))
        assert bad.size == 0, (what, name, len(bad), "first query", int(bad[0, 0]), got[bad[0, 0]], want[bad[0, 0]])


# 1. the device arithmetic, bit for bit
@pytest.mark.parametrize("res", [1, 2, 3, 16, 64])
@pytest.mark.parametrize("kind", ["peaked", "banded", "equal"])
def test_batch_equals_the_mirror(gpu_pkg, batch_renderer, kind, res):
    img = M.make_image(kind, res, 100 + res)
    for name, m in XFORMS.items():
        light = M.EnvLight(img, SKY_L, m)
        d, u = M.make_queries(light, N, res)
        if m is not None:     # the exact directions are exact in LIGHT space: send their images under the transform
            d[:32] = M.xform(light.m, d[:32])
        batch_renderer.set_environment_image(0, img, m)
        got = batch_renderer.envlight_batch(0, d, u)
        want = light.batch(d, u)
        if name == "identity":     # the exact cases are among the queries: u == 1 and v == 1, a variate on a CDF entry
            assert (want[:, 3] == 1).any() and (want[:, 4] == 1).any() and np.isin(u[:, 1], light.mcdf).any()
        assert_batch_equals_mirror(got, want, (kind, res, name))


def test_average_is_rounded_to_float_on_the_host(gpu_pkg, batch_renderer):
    """The image of tests/test_envlight_model.py::test_average_is_rounded_to_float_before_it_is_subtracted, whose tables are derived by
    hand there: PDF_Li is 4 / (4 pi) in texel (row 1, column 1) and 0 in (row 1, column 0), which a double average would make samplable;
    every sample lands in the former."""
    img = M.rounded_average_image()
    light = M.EnvLight(img, SKY_L)
    assert light.func.tolist() == [[0, 0], [0, 2.0 ** -22]]
    batch_renderer.set_environment_image(0, img, None)
    d = M.square_to_sphere(np.array([0.25, 0.75], f32), np.array([0.75, 0.75], f32))
    q, u = M.make_queries(light, 256, 9)
    q[:2] = d
    got = batch_renderer.envlight_batch(0, q, u)
    assert got[0, 5] == 0 and got[1, 5] == f32(4) / f32(f32(4) * M.PI)
    ok = got[:, 6] == 1
    assert ok.sum() > 200 and np.all(got[ok, 7:9] >= 0.5) and np.all(got[ok, 12] == got[1, 5])
    assert_batch_equals_mirror(got, light.batch(q, u), "rounded average")


# 2. valid from creation on: the 1 x 1 white image under the identity
def test_created_without_an_image_is_the_white_texel(gpu_pkg):
    r = gpu_pkg.Renderer(sky_only_scene(gpu_pkg), gpu_pkg.app_f_params(), 8, 8)
    light = M.EnvLight(np.ones((1, 1, 3), f32), SKY_L)
    d, u = M.make_queries(light, N, 1)
    got = r.envlight_batch(0, d, u)
    assert_batch_equals_mirror(got, light.batch(d, u), "as created")
    assert np.all(got[:, 0:3] == np.array(SKY_L, f32)) and np.all(got[:, 5] == f32(1) / f32(f32(4) * M.PI)) and np.all(got[:, 6] == 1)
    r.render_wave(0, 1)
    film = r.film()
    assert np.all(film[..., :3] == np.array(SKY_L, f32)) and np.all(film[..., 3] == 1)
    r.close()


# 3. kernel families
def peaked_sky():
    return M.make_image("peaked", 16, 11)


def homogeneous_ground_scene(P):
    s = scenes.empty_scene(W, H, eye=(0, 0.3, -3), look=(0, 0, 0))
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (0.05, 0.05, 0.05)
    m.sigma_s[:] = (0.4, 0.4, 0.4)
    m.g = 0.3
    tp, tk = scenes.heightfield_triangles(4, x0=-4, x1=4, z0=-4, z1=4, y=-0.8)
    P.set_triangles(s, tp, tk)
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    P.add_infinite_light(s, P.LIGHT_DISTANT, (3.0, 2.5, 2.0), (0.4, 0.8, -0.3))
    return s


def grid_scene(P, boundary):
    dens = np.array([0.2, 1, 0.7, 0.1, 0.9, 0.4, 1, 0.6], f32)
    if boundary:
        s = scenes.cloud_scene(W, H, dens, 2, sigma_t=3.0, albedo=0.99, g=0.6, sphere=True, ground=True, sun=True, sky=False)
    else:       # the medium's box in a scene it fills: the camera is in the medium, outside the box the density is zero
        s = scenes.empty_scene(W, H, eye=(0.0, 0.6, -4.2), look=(0, 0.15, 0), fov=38.0)
        m = s.medium
        m.type = P.MEDIUM_GRID
        m.sigma_a[:] = (0.03,) * 3
        m.sigma_s[:] = (2.97,) * 3
        m.g = 0.6
        m.nx = m.ny = m.nz = 2
        m.bounds_min[:] = (-0.8, -0.5, -0.8)
        m.bounds_max[:] = (0.8, 0.9, 0.8)
        import ctypes as C
        m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
        s._density_keepalive = dens
        scenes.add_quad(s, (-6, -1.2, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))
        P.add_infinite_light(s, P.LIGHT_DISTANT, (6.0, 5.5, 5.0), (0.4, 0.8, -0.3))
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    return s


def sky_index(scene, P):
    return [k for k in range(scene.n_infinite_lights) if scene.infinite_lights[k].type == P.LIGHT_IMAGE_INFINITE][0]


def render(P, scene, prm, kernel, waves=4, image=None, m=None):
    def go():
        r = P.Renderer(scene, prm, W, H)
        if image is not None:
            r.set_environment_image(sky_index(scene, P), image, m)
        name = r.kernel_name()
        for w in range(waves):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        film = r.film()
        r.close()
        return name, film
    return with_kernel(kernel, go)


@pytest.mark.parametrize("sampler", ["uniform", "power", "bvh"])
@pytest.mark.parametrize("which", ["homogeneous", "grid", "grid_boundary"])
def test_kernel_families_agree(gpu_pkg, which, sampler):
    P = gpu_pkg
    scene = homogeneous_ground_scene(P) if which == "homogeneous" else grid_scene(P, which == "grid_boundary")
    prm = P.app_f_params()
    prm.lightsampler = {"uniform": P.LIGHTSAMPLER_UNIFORM, "power": P.LIGHTSAMPLER_POWER, "bvh": P.LIGHTSAMPLER_BVH}[sampler]
    name_d, film_d = render(P, scene, prm, None, image=peaked_sky(), m=rotation())
    name_l, film_l = render(P, scene, prm, "lane", image=peaked_sky(), m=rotation())
    print(which, sampler, "default:", name_d, "| lane:", name_l)
    assert name_d != name_l and name_l.startswith("k_render_wave<")
    assert np.isfinite(film_d).all() and film_d[..., :3].max() > 0
    assert np.array_equal(u32(film_d), u32(film_l))


# 4. a known answer through the whole path
def test_constant_sky_through_an_empty_medium(gpu_pkg):
    P = gpu_pkg
    s = scenes.empty_scene(W, H, eye=(0, 0.2, -3), look=(0, 0, 0))
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (0, 0, 0)
    m.sigma_s[:] = (0, 0, 0)
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    c = np.array([0.75, 0.5, 2.0], f32)
    img = np.broadcast_to(c, (3, 3, 3)).copy()
    for kernel in (None, "lane"):
        def go():
            r = P.Renderer(s, P.app_f_params(), W, H)
            r.set_environment_image(0, img, rotation())
            r.render_wave(0, 1)
            f = r.film()
            r.close()
            return f
        film = with_kernel(kernel, go)
        assert np.all(film[..., 3] == 1)
        assert np.array_equal(u32(film[..., :3]), u32(np.broadcast_to(c * np.array(SKY_L, f32), (H, W, 3)))), kernel


# 5. unbiased: NEE + MIS against escaping rays alone
def test_nee_agrees_with_escaped_rays_only(gpu_pkg):
    """Whole-film means of 32 separately cleared waves with NEE and 32 with usenee false (no light pdf enters: escaped rays carry the
    sky unweighted), compared by Welch's statistic: |z| <= 4.5, a probability condition with a false alarm of about 7e-6, not a measured
    tolerance.  The sky is envlight_model.unbiased_sky() (peak factor 30), chosen on the CPU by
    tests/test_envlight_model.py::test_planted_errors_shift_the_estimators_expectation: in its model problem a missing / (4 pi) and an
    uncompensated sampler each move the NEE arm by more than ten times what the statistic allows.  The only light is the sky, so nothing
    dilutes the shift."""
    P = gpu_pkg
    scene = grid_scene(P, False)
    scene.n_infinite_lights = 0
    P.add_infinite_light(scene, P.LIGHT_IMAGE_INFINITE, SKY_L)
    means = {}
    for nee in (1, 0):
        prm = P.app_f_params()
        prm.usenee = nee
        r = P.Renderer(scene, prm, W, H)
        r.set_environment_image(0, M.unbiased_sky(), rotation())
        ms = []
        for w in range(32):
            r.film_clear()
            r.render_wave(w, w + 1)
            f = r.film()
            ms.append(float((f[..., :3].astype(np.float64).sum(axis=2) / 3).mean()))
        r.close()
        means[nee] = np.array(ms)
    a, b = means[1], means[0]
    z = (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("NEE %.5f +- %.5f, escaped only %.5f +- %.5f, z = %.3f" % (a.mean(), a.std(ddof=1) / math.sqrt(32), b.mean(), b.std(ddof=1) / math.sqrt(32), z))
    assert abs(z) <= 4.5, z


# 6. set_environment_image on a live renderer
def test_set_image_on_a_live_renderer(gpu_pkg):
    P = gpu_pkg
    scene = grid_scene(P, True)
    k = sky_index(scene, P)
    prm = P.app_f_params()
    prm.lightsampler = P.LIGHTSAMPLER_POWER
    prm.vspguiding = 0
    first, second = M.make_image("banded", 16, 5), peaked_sky()
    r = P.Renderer(scene, prm, W, H)
    r.set_environment_image(k, first, None)
    r.render_wave(0, 1)
    r.post_process_wave()
    film1, cnt1 = r.film(), r.counters()
    r.set_environment_image(k, second, rotation())
    assert np.array_equal(u32(r.film()), u32(film1)) and r.counters() == cnt1      # film and counters survive the call
    light = M.EnvLight(second, SKY_L, rotation())
    d, u = M.make_queries(light, 512, 2)
    assert_batch_equals_mirror(r.envlight_batch(k, d, u), light.batch(d, u), "second image replaces the first")
    # every refusal leaves the renderer as it was
    bad = second.copy()
    bad[3, 4, 1] = np.nan
    inf = second.copy()
    inf[0, 0, 0] = np.inf
    sing = rotation((1, 0, 1))
    fp = P.C.POINTER(P.C.c_float)
    raw = lambda idx, img, res, m: r.lib.vspg_renderer_set_environment_image(r.h, idx, img.ctypes.data_as(fp) if img is not None else None, res,
                                                                             m.ctypes.data_as(fp) if m is not None else None, None)
    other = [i for i in range(scene.n_infinite_lights) if i != k][0]
    for args, words in (((other, second, 16, None), b"not of type"), ((7, second, 16, None), b"names no infinite light"), ((k, second, 0, None), b"resolution"),
                        ((k, second, 4097, None), b"resolution"), ((k, None, 16, None), b"null"), ((k, bad, 16, None), b"not-a-number"),
                        ((k, inf, 16, None), b"infinite pixel"), ((k, second, 16, sing), b"singular")):
        assert raw(*args) == P.VSPG_EINVAL and words in r.lib.vspg_last_error(), (words, r.lib.vspg_last_error())
    assert_batch_equals_mirror(r.envlight_batch(k, d, u), light.batch(d, u), "after the refusals")
    r.film_clear()
    r.render_wave(0, 2)
    film_upd = r.film()
    r.close()
    fresh = P.Renderer(scene, prm, W, H)       # (no VSP guiding: a wave does not depend on the waves before it)
    fresh.set_environment_image(k, second, rotation())
    fresh.render_wave(0, 2)
    film_fresh = fresh.film()
    fresh.close()
    assert film_upd[..., :3].max() > 0 and np.isfinite(film_upd).all()
    assert np.array_equal(u32(film_upd), u32(film_fresh))


def test_set_image_equals_a_renderer_given_it_directly(gpu_pkg):
    """A -> B on a live renderer before any wave renders as a renderer given B directly, bit for bit; the guiding fields of a training
    renderer survive the call."""
    P = gpu_pkg
    scene = grid_scene(P, True)
    k = sky_index(scene, P)
    prm = P.app_f_params()
    prm.lightsampler = P.LIGHTSAMPLER_POWER
    a, b = M.make_image("banded", 16, 5), peaked_sky()
    films = []
    for seq in ((a, b), (b,)):
        r = P.Renderer(scene, prm, W, H)
        for img in seq:
            r.set_environment_image(k, img, rotation())
        for w in range(3):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        films.append(r.film())
        r.close()
    assert np.array_equal(u32(films[0]), u32(films[1]))
    g = P.default_params()
    r = P.Renderer(scene, g, W, H)
    r.set_environment_image(k, a, None)
    for w in range(3):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    def fields():      # both fields as the device holds them: nodes and regions, byte for byte
        out = []
        for vol in (0, 1):
            nodes, regs, nn, nr = r.get_guiding_field(vol)
            out.append((nn, nr, bytes(nodes)[:nn * P.C.sizeof(P.VspgKdNode)], bytes(regs)[:nr * P.C.sizeof(P.VspgFieldRegion)]))
        return out
    before, fields_before = r.training_stats(), fields()
    assert before["iteration"] >= 1 and max(f[1] for f in fields_before) >= 1
    r.set_environment_image(k, b, rotation())
    assert r.training_stats() == before
    assert fields() == fields_before
    r.close()


# 7. guided, training in the loop
def test_guided_training_runs_and_kernels_agree(gpu_pkg):
    """In-loop training under the image sky: four waves run and stay finite, the field grows.  The kernels are then compared as
    tests/test_gpu_parity.py compares guided kernels: with that field and that VSP buffer in place, wave 4 on the pipeline and on the
    per-lane kernel, bit for bit.  (Films of two in-loop TRAINING runs on different kernels are not comparable bit for bit with any
    light: the radiance samples reach the update in an unspecified order -- include/vspg.h, vspg_train_samples_read -- and its float
    sums follow that order.  Measured here with the sky: the two trained films differ in the last bits from the first update on.)
    The first wave, recorded with the field still empty, gives both kernels the same samples as a set, the escaped rays' among them."""
    P = gpu_pkg
    scene = grid_scene(P, True)
    k = sky_index(scene, P)
    prm = P.default_params()
    prm.guide_num_training_waves = 4
    samples = {}
    for kernel in (None, "lane"):
        def first_wave():
            r = P.Renderer(scene, prm, W, H)
            r.set_environment_image(k, peaked_sky(), rotation())
            r.render_wave(0, 1)
            smp = r.train_samples()
            name = r.kernel_name()
            r.close()
            rows = np.frombuffer(np.ascontiguousarray(smp).tobytes(), dtype=np.uint32).reshape(len(smp), -1)
            return name, rows[np.lexsort(rows.T)]
        name, samples[kernel] = with_kernel(kernel, first_wave)
        assert "train" in name, name
    assert len(samples[None]) > 100 and samples[None].tobytes() == samples["lane"].tobytes()
    t = P.Renderer(scene, prm, W, H)
    t.set_environment_image(k, peaked_sky(), rotation())
    for w in range(4):
        t.render_wave(w, w + 1)
        t.post_process_wave()
    assert np.isfinite(t.film()).all() and t.film()[..., :3].max() > 0
    st = t.training_stats()
    assert st["training"] == 0 and st["iteration"] == 4, st
    fields = []
    for vol in (0, 1):
        nodes, regs, nn, nr = t.get_guiding_field(vol)
        fields.append(P.Field(list(nodes)[:nn], list(regs)[:nr]))
    vsp, ready = t.vsp_buffer()
    t.close()
    films = {}
    for kernel in (None, "lane"):
        def wave4():
            r = P.Renderer(scene, prm, W, H)
            r.set_environment_image(k, peaked_sky(), rotation())
            r.set_guiding_field(fields[0], fields[1])
            if ready:
                r.load_vsp_buffer(vsp)
            r.render_wave(4, 5)
            name, film = r.kernel_name(), r.film()
            r.close()
            return name, film
        name, film = with_kernel(kernel, wave4)
        films[name] = film
    print("guided kernels compared:", sorted(films))
    assert len(films) == 2 and any(n.startswith("k_render_wave<") for n in films)
    fa, fb = films.values()
    assert np.isfinite(fa).all() and fa[..., :3].max() > 0
    assert np.array_equal(u32(fa), u32(fb))


# 8. the scene-file route
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")


@pytest.fixture(scope="module")
def exe(gpu_pkg):
    import subprocess
    subprocess.check_call(["make", "-C", HOST])
    return os.path.join(HOST, "vspg_pbrt")


def sky_scene_text(filename, extra=""):
    """tests/scenes/fog_box.pbrt with its back wall taken out (rays leave the box through it) and an image sky under a Rotate."""
    lines = open(os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")).read().splitlines()
    kept = [l for l in lines if "# back  z = +1" not in l]
    assert len(kept) == len(lines) - 1
    sky = ['AttributeBegin', '  Rotate 40 0 1 0', '  LightSource "infinite" "string filename" "%s" "float scale" 0.8 %s' % (filename, extra), 'AttributeEnd']
    at = [i for i, l in enumerate(kept) if l.startswith("WorldBegin")][0]
    return "\n".join(kept[:at + 1] + sky + kept[at + 1:]) + "\n"


def rotate_y(deg):
    """The scene-file reader's Rotate about (0, 1, 0) (transform.h:220-247 in float): rows of the 3 x 4 matrix."""
    rad = f32(f32(M.PI / f32(180)) * f32(deg))
    s, c = M.sinf([rad])[0], M.cosf([rad])[0]
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0]], f32)


def test_scene_file_image_sky(gpu_pkg, exe, tmp_path):
    import subprocess
    import exr_model as X
    P = gpu_pkg
    img = M.make_image("peaked", 16, 21, peak=50)
    X.write_exr(str(tmp_path / "sky.exr"), {c: np.ascontiguousarray(img[..., i]).view(np.uint32) for i, c in enumerate("RGB")}, pixel_type=X.FLOAT)
    X.write_pfm(str(tmp_path / "sky.pfm"), img)
    films = {}
    for ext in ("exr", "pfm"):
        scene = tmp_path / ("sky_%s.pbrt" % ext)
        scene.write_text(sky_scene_text("sky." + ext))
        out = tmp_path / ("o_%s.pfm" % ext)
        a = subprocess.run([exe, str(scene), "--outfile", str(out), "--spp", "3"], capture_output=True, text=True, timeout=120)
        assert a.returncode == 0, a.stdout + a.stderr
        films[ext] = X.read_pfm(str(out))
    assert np.array_equal(u32(films["exr"]), u32(films["pfm"]))
    # the same render through the C-ABI: the fog box without its back wall (rectangle 2), the sky under the same rotation
    s = P.fog_box_scene(64, 48)
    for i in range(2, s.n_quads - 1):
        s.quads[i] = s.quads[i + 1]
    s.n_quads -= 1
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, (0.8, 0.8, 0.8))
    r = P.Renderer(s, P.app_f_params(), 64, 48)
    r.set_environment_image(0, img, rotate_y(40))
    for w in range(3):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    f = r.film()
    r.close()
    want = (f[..., :3] / f[..., 3:4]).astype(f32)
    assert want.max() > 0 and np.array_equal(u32(films["exr"]), u32(want))
    # refusals, each by name
    grey = np.ascontiguousarray(img[..., 0])
    X.write_exr(str(tmp_path / "grey.exr"), {"Y": grey.view(np.uint32)}, pixel_type=X.FLOAT)
    X.write_pfm(str(tmp_path / "wide.pfm"), np.concatenate([img, img], axis=1))
    for text, words in ((sky_scene_text("sky.exr", '"rgb L" [ 1 1 1 ]'), 'both emission "L" and "filename"'),
                        (sky_scene_text("grey.exr"), "must have R, G, and B channels"),
                        (sky_scene_text("wide.pfm"), "is non-square"),
                        (sky_scene_text("sky.exr", '"point3 portal" [ 0 0 0  1 0 0  1 1 0  0 1 0 ]'), '"portal"'),
                        (sky_scene_text("sky.exr", '"float illuminance" 100'), '"illuminance"')):
        bad = tmp_path / "bad.pbrt"
        bad.write_text(text)
        b = subprocess.run([exe, str(bad), "--parse-only"], capture_output=True, text=True, timeout=60)
        assert b.returncode == 1 and words in b.stderr, (words, b.stderr)
