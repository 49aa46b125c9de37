"""Diagnostic: ms per 1080p wave of the fog box with two more rectangles in the room, next to the fog box itself -- the price of the
any-hit walk's pre-pass (csrc/vspg_device.h, rects_any_planes) where it cannot end the walk: a shelf across the room and a screen
beside it put a plane in front of most shadow rays, so some lane of nearly every wavefront is a candidate of some record, the
pre-pass is pure overhead and the walk over the voted records follows it.  Run it once per library (VSPG_LIB), alternated.

    python scripts/occluder_timing.py [rounds]"""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import torch
import __graft_entry__ as g
P = g.load_package(); P.load()
W, H = 1920, 1080
def scene(occluders):
    s = P.fog_box_scene(W, H)
    if occluders:
        P.add_quad(s, (-0.7, 0.3, -0.2), (0, 0, 0.9), (1.0, 0, 0))      # a shelf under the light, facing down
        P.add_quad(s, (0.5, -0.8, -0.3), (0, 1.1, 0), (0, 0, 1.0))      # a screen beside it
    return s
def run(label, occluders):
    r = P.Renderer(scene(occluders), P.app_f_params(), W, H)
    for w in range(4): r.render_wave(w, w + 1); r.post_process_wave()
    torch.cuda.synchronize(); r.reset_counters()
    t0 = time.perf_counter()
    n = 32
    for w in range(4, 4 + n): r.render_wave(w, w + 1)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    c = r.counters()
    print("%-14s %s  %.4f ms/wave  segments/path %.2f shadow/path %.2f" % (label, r.kernel_name()[:24], dt * 1e3, c["segments"] / max(1, c["paths"]), c["shadow_rays"] / max(1, c["paths"])))
    r.close()
for k in range(int(sys.argv[1]) if len(sys.argv) > 1 else 1):
    run("fog box", False)
    run("two occluders", True)
