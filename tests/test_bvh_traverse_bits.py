"""The triangle traversal (csrc/vspg_device.h: bvh_box_hit, bvh_traverse, bvh_closest, bvh_any) answers what a brute-force walk over all
triangles answers, bit for bit, on the rays that touch its edge cases; no GPU needed.

The header carries two statements about the traversal: "which boxes are visited never changes a result", and that a NaN in the slab
test (0 * inf: the ray runs along a box face) keeps the node.  The oracle has no BVH -- it walks all triangles and gives ties to the
smaller id -- and device == oracle is held bit for bit on every query, so the traversal's contract is brute force.  Films and replays
see triangles through a jittered pinhole camera: no ray of theirs has a direction component of exactly zero or an origin exactly on
a box face.

The header's text from TriHit to bvh_any is cut out as it stands, with the few helpers it uses (V3, ld3, operator-, vabs,
diff_of_products, fmax_, fmin_, comp: cut out too), and compiled for the host as `static inline` inside tests/bvh_traverse_check.cpp with
the library's own flags (csrc/Makefile: HIPFLAGS).  DTri, DBvh4Node, DScene, kBvhStack and kBvhAbsent come from the header itself, and every
tree from build_triangle_bvh (csrc/vspg_scene_build.hip, linked in as tests/test_scene_build.py links it).  The program has its own main
and is built with AddressSanitizer and UndefinedBehaviorSanitizer -- the stack arrays st_ref[kBvhStack] and st_t sit between red zones --
and run directly; nothing is loaded into Python.  Two counters are inserted by textual replacement (each exactly once): the stack's
high-water mark behind the one `sp++;`, and a visit counter at the head of the loop that stops a query which visits more nodes and
leaves than the tree has (the traversal visits each at most once, so it terminates; rays with infinities and NaNs are among the inputs).

Per ray: found / not found, the winner's id and the bits of t, b0, b1, b2 of bvh_closest, and the boolean of bvh_any, against a loop
over all accepted triangles with the same tri_intersect and the RAY's tMax, the closest decided by (t, id).  No ray may differ in any
family (see the driver for each): flat grids in a plane of each axis with perpendicular rays through every vertex, edge midpoint and
cell centre and +0 / -0 in all sign combinations, with tMax at the hit distance (a miss) and one float above (a hit), and rays in the
grid's plane (misses); axis-parallel rays onto tilted triangles; two layers; nine and fourteen coincident copies with shuffled ids (the
smallest id wins -- asserted on its own as well; identical centroids force the median split: nine give leaves of 4 and 5, fourteen two
full leaves of 7) and two triangulations of one plane; soups of 1, 2, 3, 7, 8, 9; 1000 triangles in one box; stacked sheets; the
cascade at x = 2^-k; a random soup with random rays, zeros, denormals, infinities and NaNs; slivers at grazing angles; a soup of
coordinates +-10^(-4..4) with aimed rays.  Stack occupancy: at most 3 x the four-wide depth and kBvhStack per family, and some family
must reach 16 entries (the wide-range soup reaches 21 at depth 12, the slivers 19, the cascades 18).

Found by this test, besides the NaN of (a): the culling slack applied to the closest hit so far but not to the ray's own tMax.  With
the two layers (every box flat: entry distance == hit distance) and tMax one float above the hit distance, the slab's distance to a
flat box came out three floats ABOVE the triangle test's t, so above tMax: the box was dropped and the hit lost, for bvh_closest and
bvh_any alike (28 of 17 154 rays).  `lim` carries the slack against tMax too now; plant (d) is that bug and the older half of it.

Planted errors, each built from the patched text and required to fail with its counts printed:
  (a) the slab test as it was before this test existed (no NaN guard): 832 closest hits of the first family's 1156 rays differ, 132 of
      them hit / miss, 132 any-hit answers; the same counts with x or y in the flat role;
  (b) the tie-break `T.id < best_id` removed;
  (c) a leaf's count read as `& 3`.
Tried and reported, not required (no family was tuned for them); both are caught:
  (d) the culling slack 1.00001f on `lim` removed: two layers with tMax at the hit distance 28 (all hit / miss), two triangulations of
      one plane 48, 1000 triangles in one box 273, cascade of 126 48 (other winners);
  (e) triangles tested against the running `limit` instead of the ray's tMax: 19 families differ, never in hit / miss (equal t: the
      copy that comes second fails `tScaled > limit * det` or `h.t < limit` and the smaller id loses)."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
HDR = os.path.join(CSRC, "vspg_device.h")
DRIVER = os.path.join(ROOT, "tests", "bvh_traverse_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
UNITS = ("vspg_scene_build", "vspg_scene_api")

GUARD = "    if (GUARD && __builtin_isunordered(a, b)) return;\n"
PLANTS = {
    "a": (GUARD, ""),
    "b": ("(h.t == best->t && T.id < best_id)", "(h.t == best->t)"),
    "c": ("cnt = leaf & 7;", "cnt = leaf & 3;"),
    "d": ("const float lim = limit * 1.00001f;", "const float lim = limit;"),
    "e": ("if (tri_intersect(o, R, tMax, ld3(T.p0), ld3(T.p1), ld3(T.p2), &h) && h.t < tMax) {",
          "if (tri_intersect(o, R, limit, ld3(T.p0), ld3(T.p1), ld3(T.p2), &h) && h.t < limit) {"),
}


def _cut(src, pattern, what):
    m = re.search(pattern, src, re.S | re.M)
    assert m, "%s not found" % what
    return m.group(0)


def _line(src, start):
    return _cut(src, r"^%s[^\n]*\n" % re.escape(start), start)


def _replace_once(text, old, new):
    assert text.count(old) == 1, "%r occurs %d times" % (old, text.count(old))
    return text.replace(old, new)


def traversal_text(header):
    """The traversal's text and its helpers as the header has them, with the two counters inserted."""
    helpers = "".join([_cut(header, r"^struct V3 \{.*?^};\n", "struct V3"), _line(header, "VDEV V3 ld3("), _line(header, "VDEV V3 operator-(V3 a, V3 b)"),
                       _line(header, "VDEV V3 vabs("), _cut(header, r"^VDEV float diff_of_products\(.*?^}\n", "diff_of_products"),
                       _line(header, "VDEV float fmax_("), _line(header, "VDEV float fmin_("), _line(header, "VDEV float comp(")])
    body = _cut(header, r"^struct TriHit \{.*?^VDEV bool bvh_any\(.*?^}\n", "TriHit ... bvh_any")
    assert "asm" not in body and "#if" not in body
    body = _replace_once(body, "sp++;", "sp++; if (sp > g_high_water) g_high_water = sp;")
    body = _replace_once(body, "    while (true) {\n", "    while (true) {\n        if (++g_steps > g_step_cap) { g_runaway = true; return false; }\n")
    return helpers, body


def _run(cmd, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return p


class Build:
    """The two host units once, and one program per text: the header's own ("") and one per plant."""

    def __init__(self, tmp, header):
        self.tmp = tmp
        self.hipcc = os.path.join(ROCM, "bin", "hipcc")
        self.clangxx = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
        for tool in (self.hipcc, self.clangxx):
            if not os.path.exists(tool):
                pytest.fail("%s not found (ROCm)" % tool)
        flags = shlex.split(_run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"]).stdout)
        assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags, flags
        self.flags = flags + [a for s in SANITIZE for a in ("-Xarch_host", s)] + ["-g"]
        self.helpers, self.body = traversal_text(header)
        jobs = [self._compile(os.path.join(CSRC, u + ".hip"), str(tmp / (u + ".o")), []) for u in UNITS]
        self.unit_objs = [j[2] for j in jobs]
        texts = {"": self.body}
        self.unplantable = {}   # a plant whose place the header no longer has fails its own test, not the comparison's
        for name, (old, new) in PLANTS.items():
            try:
                texts[name] = _replace_once(self.body, old, new)
            except AssertionError as e:
                self.unplantable[name] = str(e)
        drivers = {}
        for name, body in texts.items():
            d = tmp / ("text_" + (name or "header"))
            d.mkdir()
            (d / "bvh_traverse_text.inc").write_text(self.helpers + body)
            drivers[name] = self._compile(DRIVER, str(d / "check.o"), ["-x", "hip", "-I", CSRC, "-I", str(d)])
        self.exe = {}
        for cmd, p, obj in jobs + list(drivers.values()):
            out = p.communicate()[0]
            assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
            assert b"__CLANG_OFFLOAD_BUNDLE__" not in open(obj, "rb").read(), obj  # host code only: links without the HIP runtime
        for name, (_, _, obj) in drivers.items():
            self.exe[name] = os.path.join(os.path.dirname(obj), "bvh_traverse_check")
            _run([self.clangxx] + SANITIZE + ["-o", self.exe[name], obj] + self.unit_objs)
        self._plants = None

    def _compile(self, src, obj, extra):
        cmd = [self.hipcc] + self.flags + extra + ["-c", "-o", obj, src]
        return cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), obj

    def plants(self):
        """Every planted program run once, side by side: {name: (exit status, stdout, stderr)}"""
        if self._plants is None:
            procs = {n: subprocess.Popen([self.exe[n]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for n in PLANTS if n in self.exe}
            self._plants = {}
            for n, p in procs.items():
                out, err = p.communicate(timeout=600)
                self._plants[n] = (p.returncode, out, err)
        return self._plants


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return Build(tmp_path_factory.mktemp("bvh_traverse"), open(HDR).read())


FAMILY = re.compile(r"^family (.*?): triangles (\d+) nodes (\d+) depth (\d+) rays (\d+) hits (\d+) high-water (\d+) closest-mismatches (\d+) "
                    r"hit-miss-mismatches (\d+) any-mismatches (\d+)$", re.M)


def _families(out):
    return [(m.group(1),) + tuple(int(v) for v in m.groups()[1:]) for m in FAMILY.finditer(out)]


def test_traversal_equals_brute_force_on_every_ray_and_is_clean_under_sanitizers(built):
    p = subprocess.run([built.exe[""]], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert p.stderr.strip() == "", p.stderr
    assert "result identical" in p.stdout
    fams = _families(p.stdout)
    assert len(fams) >= 30, len(fams)
    for name, tris, nodes, depth, rays, hits, high, closest, hitmiss, anyhit in fams:
        assert (closest, hitmiss, anyhit) == (0, 0, 0), name
        assert rays > 0 and high <= min(3 * depth, 48), name
    assert max(f[6] for f in fams) >= 16   # some family fills a third of the stack


def _plant(built, name):
    assert name not in built.unplantable, built.unplantable[name]
    status, out, err = built.plants()[name]
    fams = _families(out)
    assert fams, "%s\n%s" % (out, err)
    bad = [(f[0], f[7], f[8], f[9]) for f in fams if f[7] or f[8] or f[9]]
    print("plant (%s): %d mismatching families of %d" % (name, len(bad), len(fams)))
    for b in bad:
        print("  %s: closest %d (hit / miss %d), any-hit %d" % b)
    for line in re.findall(r"^.*winners are not the smallest id.*$", out, re.M):
        print(line)
    return status, out, fams, bad


def test_plant_a_the_slab_test_without_the_nan_guard_fails(built):
    status, out, fams, bad = _plant(built, "a")
    assert status != 0 and "result MISMATCH" in out
    first = fams[0]
    assert first[0] == "flat grid z, perpendicular, zeros of one sign" and first[4] == first[5] == 1156
    assert (first[7], first[8], first[9]) == (832, 132, 132), first   # the counts of the report that asked for this test
    for ax in "xy":   # each axis in the flat role
        assert any(b[0] == "flat grid %s, perpendicular, zeros of one sign" % ax and b[1] > 0 and b[2] > 0 and b[3] > 0 for b in bad)


def test_plant_b_no_tie_break_by_id_fails(built):
    status, out, fams, bad = _plant(built, "b")
    assert status != 0 and "result MISMATCH" in out
    for copies in (9, 14):
        assert any(b[0] == "ties, %d coincident copies" % copies and b[1] > 0 for b in bad), bad
    assert not re.search(r": 0 winners are not the smallest id", out)
    assert all(b[2] == 0 and b[3] == 0 for b in bad), bad   # the same hits, other winners


def test_plant_c_leaf_count_of_two_bits_fails(built):
    status, out, fams, bad = _plant(built, "c")
    assert status != 0 and "result MISMATCH" in out
    assert sum(b[1] for b in bad) > 0 and sum(b[3] for b in bad) > 0, bad


def test_plants_d_and_e_are_caught_too(built):
    """Tried without any family made for them (the module's docstring has what they gave); both differ from brute force."""
    status, out, fams, bad = _plant(built, "d")
    assert status != 0 and "result MISMATCH" in out
    assert any(b[0] == "two layers, tMax at the hit distance" and b[2] > 0 and b[3] > 0 for b in bad), bad
    status, out, fams, bad = _plant(built, "e")
    assert status != 0 and "result MISMATCH" in out
    assert sum(b[1] for b in bad) > 0 and all(b[2] == 0 and b[3] == 0 for b in bad), bad
