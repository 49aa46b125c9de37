"""Film "cropwindow" / "pixelbounds" and --cropwindow / --pixelbounds through `vspg_pbrt --parse-only`: the resolved pixel bounds
follow the reference's rules (film.cpp:97-172, cmd/pbrt.cpp:132-153).  The expected bounds are computed here from those rules:
ceil(resolution * crop) in float32 (`Float` is `float`), corners ordered per axis, the crop window clamped to [0,1], pixel bounds
clamped to the frame with a warning, the command line over the file, a crop window over pixel bounds."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host", "vspg_pbrt")
f32 = np.float32

SCENE = """LookAt 0 0 -0.95   0 0 0   0 1 0
MediumInterface "" "fog"
Camera "perspective" "float fov" 60
Sampler "independent" "integer pixelsamples" 1
Film "rgb" "integer xresolution" %d "integer yresolution" %d "string filename" "w.pfm" %s
Integrator "guidedvolpathvspg" "integer maxdepth" 5 "bool vspguiding" true "bool surfaceguiding" false
    "bool volumeguiding" false "bool vspsecondaryguiding" false
WorldBegin
MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [ .05 .05 .05 ] "rgb sigma_s" [ .45 .45 .45 ] "float g" 0
MediumInterface "fog" "fog"
Material "diffuse" "rgb reflectance" [ .73 .73 .73 ]
Shape "bilinearmesh" "point3 P" [ -1 -1 -1   -1 -1 1    1 -1 -1    1 -1 1 ]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 17 12 4 ]
  Shape "bilinearmesh" "point3 P" [ -0.25 0.999 -0.25   0.25 0.999 -0.25   -0.25 0.999 0.25   0.25 0.999 0.25 ]
AttributeEnd
"""


def crop_rule(res, crop):
    """film.cpp:134-137 / 157-166 -> (x0, y0, x1, y1)"""
    c = [f32(v) for v in crop]
    cl = lambda v: min(max(v, f32(0)), f32(1))
    x0, x1, y0, y1 = cl(min(c[0], c[1])), cl(max(c[0], c[1])), cl(min(c[2], c[3])), cl(max(c[2], c[3]))
    ce = lambda r, v: int(math.ceil(f32(f32(r) * v)))
    return ce(res[0], x0), ce(res[1], y0), ce(res[0], x1), ce(res[1], y1)


def bounds_rule(res, pb):
    """film.cpp:99-120 -> (x0, y0, x1, y1), clamped?"""
    x0, x1, y0, y1 = min(pb[0], pb[1]), max(pb[0], pb[1]), min(pb[2], pb[3]), max(pb[2], pb[3])
    out = (max(x0, 0), max(y0, 0), min(x1, res[0]), min(y1, res[1]))
    return out, out != (x0, y0, x1, y1)


def run(tmp_path, res, film_params="", *args):
    path = tmp_path / "scene.pbrt"
    path.write_text(SCENE % (res[0], res[1], film_params))
    p = subprocess.run([EXE, str(path), "--parse-only"] + list(args), capture_output=True, text=True, timeout=120)
    m = re.search(r"pixel bounds: \[ \((-?\d+), (-?\d+)\) - \((-?\d+), (-?\d+)\) \]", p.stdout)
    return p, tuple(int(v) for v in m.groups()) if m else None


def arr(kind, name, vals):
    return '"%s %s" [ %s ]' % (kind, name, " ".join(repr(float(v)) if kind == "float" else str(v) for v in vals))


CROPS = [((1920, 1080), (0.1, 0.7, 0.1, 0.7)),       # 1920 * 0.1f = 192.0000029 in exact arithmetic, 192 as a float: ceil gives 192
         ((1920, 1080), (0.25, 0.75, 0.5, 1.0)),     # integer products
         ((1920, 1080), (0.3, 0.6, 0.7, 0.9)),
         ((100, 76), (0.13, 0.77, 0.07, 0.66)),
         ((100, 76), (0.15, 0.6, 0.25, 0.75)),       # 100 * 0.15f and 100 * 0.6f round UP in float: 16 and 61, where double gives 15 and 60
         ((100, 76), (0.07, 0.28, 0.5, 1.0)),        # 100 * 0.07f and 100 * 0.28f land on 7 and 28, where double gives 8 and 29
         ((100, 76), (0.77, 0.13, 0.66, 0.07)),      # min / max swapped
         ((100, 76), (-0.5, 0.5, 0.25, 1.75)),       # clamped to [0, 1]
         ((3840, 2160), (0.05, 0.95, 0.35, 0.65)),
         ((7, 5), (0.2, 0.8, 0.4, 0.6))]


def test_float_rounding_matters_in_the_table():
    """the table holds products that are integers and products whose float rounding decides the ceil"""
    assert f32(1920) * f32(0.25) == 480 and crop_rule((1920, 1080), (0.25, 0.75, 0.5, 1.0)) == (480, 540, 1440, 1080)
    assert crop_rule((1920, 1080), (0.1, 0.7, 0.1, 0.7)) == (192, 108, 1344, 756)
    assert crop_rule((100, 76), (0.15, 0.6, 0.25, 0.75))[::2] == (16, 61) and (math.ceil(100 * 0.15), math.ceil(100 * 0.6)) == (15, 60)
    assert crop_rule((100, 76), (0.07, 0.28, 0.5, 1.0))[::2] == (7, 28) and (math.ceil(100 * 0.07), math.ceil(100 * 0.28)) == (8, 29)


@pytest.mark.parametrize("res,crop", CROPS)
def test_cropwindow_in_the_file_and_on_the_command_line(tmp_path, res, crop):
    want = crop_rule(res, crop)
    p, got = run(tmp_path, res, arr("float", "cropwindow", crop))
    assert p.returncode == 0 and got == want, (p.stdout, p.stderr, want)
    p, got = run(tmp_path, res, "", "--cropwindow", ",".join(repr(float(v)) for v in crop))
    assert p.returncode == 0 and got == want, (p.stdout, p.stderr, want)
    p, got = run(tmp_path, res)
    assert got == (0, 0, res[0], res[1])


@pytest.mark.parametrize("res,pb,clamped", [((100, 76), (13, 77, 5, 50), False), ((100, 76), (77, 13, 50, 5), False),
                                            ((100, 76), (-4, 130, 10, 90), True), ((1920, 1080), (0, 1920, 1079, 1080), False)])
def test_pixelbounds_in_the_file_and_on_the_command_line(tmp_path, res, pb, clamped):
    want, cl = bounds_rule(res, pb)
    assert cl == clamped
    for p, got in (run(tmp_path, res, arr("integer", "pixelbounds", pb)), run(tmp_path, res, "", "--pixelbounds", ",".join(map(str, pb)))):
        assert p.returncode == 0 and got == want, (p.stdout, p.stderr, want)
        assert ("extend beyond image resolution" in p.stderr) == clamped


def test_precedence(tmp_path):
    res = (100, 76)
    crop_f, crop_c, pb_f, pb_c = (0.1, 0.5, 0.2, 0.6), (0.3, 0.9, 0.1, 0.4), (10, 20, 30, 40), (50, 60, 1, 9)
    both = arr("float", "cropwindow", crop_f) + " " + arr("integer", "pixelbounds", pb_f)
    crop_arg, pb_arg = ",".join(map(str, crop_c)), ",".join(map(str, pb_c))
    p, got = run(tmp_path, res, both)                                   # file: the crop window over the pixel bounds
    assert got == crop_rule(res, crop_f) and "Using the crop window" in p.stderr
    p, got = run(tmp_path, res, both, "--cropwindow", crop_arg)         # command line over file
    assert got == crop_rule(res, crop_c) and "will override" in p.stderr
    p, got = run(tmp_path, res, both, "--pixelbounds", pb_arg)          # command-line pixel bounds: the file's crop window is ignored
    assert got == bounds_rule(res, pb_c)[0] and "Ignoring \"cropwindow\"" in p.stderr
    p, got = run(tmp_path, res, arr("integer", "pixelbounds", pb_f), "--pixelbounds", pb_arg)
    assert got == bounds_rule(res, pb_c)[0]
    p, got = run(tmp_path, res, "", "--pixelbounds", pb_arg, "--cropwindow", crop_arg)   # both on the command line: the crop window
    assert got == crop_rule(res, crop_c)


@pytest.mark.parametrize("film,args,msg", [
    (arr("float", "cropwindow", (0.1, 0.5, 0.2)), [], "3 values supplied for \"cropwindow\". Expected 4."),
    (arr("integer", "pixelbounds", (1, 2, 3, 4, 5)), [], "5 values supplied for \"pixelbounds\". Expected 4."),
    ("", ["--cropwindow", "0.1,0.2,0.3"], "four values after --cropwindow"),
    ("", ["--pixelbounds", "1,2"], "four integer values after --pixelbounds"),
    (arr("float", "cropwindow", (0.5, 0.5, 0.1, 0.9)), [], "Degenerate pixel bounds"),
    (arr("integer", "pixelbounds", (200, 300, 0, 10)), [], "Degenerate pixel bounds"),
    ("", ["--pixelbounds", "5,5,1,3"], "Degenerate pixel bounds"),
])
def test_wrong_value_counts_and_empty_bounds_are_errors(tmp_path, film, args, msg):
    p, got = run(tmp_path, (100, 76), film, *args)
    assert p.returncode != 0 and msg in p.stderr, (p.stdout, p.stderr)


def test_command_line_replaces_the_files_values_unexamined_and_warns_once(tmp_path):
    """With --cropwindow the file's own "cropwindow" is not examined (film.cpp:123-144): malformed there is no error; the bounds are
    resolved once, so every warning appears once; an integer option refuses a fraction instead of truncating it."""
    res = (100, 76)
    p, got = run(tmp_path, res, arr("float", "cropwindow", (0.5, 0.5, 0.1)), "--cropwindow", "0.1,0.5,0.2,0.6")
    assert p.returncode == 0 and got == crop_rule(res, (0.1, 0.5, 0.2, 0.6)), (p.stdout, p.stderr)
    assert p.stderr.count("will override") == 1
    p, got = run(tmp_path, res, arr("integer", "pixelbounds", (1, 2, 3)), "--pixelbounds", "5,50,6,60")
    assert p.returncode == 0 and got == (5, 6, 50, 60), (p.stdout, p.stderr)
    p, got = run(tmp_path, res, arr("integer", "pixelbounds", (-4, 130, 10, 90)))
    assert p.stderr.count("extend beyond image resolution") == 1
    p, got = run(tmp_path, res, arr("float", "cropwindow", (0.1, 0.5, 0.2, 0.6)) + " " + arr("integer", "pixelbounds", (10, 20, 30, 40)))
    assert p.stderr.count("Using the crop window") == 1
    p, got = run(tmp_path, res, "", "--pixelbounds", "1.5,9.9,0,4")
    assert p.returncode != 0 and "is not an integer" in p.stderr
