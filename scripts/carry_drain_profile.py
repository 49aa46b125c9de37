"""Diagnostic: what the start and the end of a one-sample k_render_wave_wg3 launch cost (needs `make -C csrc timeline`).

The timeline build records, per wavefront of the last launch, 100 MHz stamps of {loop entry, first full vertex chunk, tile cursors first
seen dry, exit} and per phase (ramp / steady / drain) and chunk kind (vertex / segment / fresh) {chunks, lanes, ticks in chunks}.  This
script renders the benchmark's sequence (1920x1080 fog box, one sample per launch, post_process_wave after each), reads the records
after every launch and prints, per launch and as medians:

  span      first loop entry -> last exit over all wavefronts (the kernel without its prologue / epilogue)
  to_exh    loop entry -> the wavefront first sees the cursors dry;  drain: from there to ITS exit;  tail: to the LAST exit
  ramp      loop entry -> the wavefront's first full vertex chunk
  ideal     the launch's chunks priced at the steady phase's ticks per lane of their kind, spread over every wavefront at the steady
            phase's share of time spent in chunks: how long the launch would last if it ran at the steady rate from end to end
  ceiling   span - ideal: the idle lane-time of ramp + drain, the most a scheme that keeps the pools full across launches can remove

and, at the end, the time per chunk of each kind in the steady phase, for the launches whose fresh chunks resolve a parked sample and for
those right behind an update of the VSP buffer (the flush resolved them: nothing parked) apart.
"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import __graft_entry__ as g
P = g.load_package()
P.LIB_PATH = os.path.join(os.path.dirname(P.LIB_PATH), "libvspg_hip_timeline.so")
lib = P.load()
W, H = 1920, 1080
WARM, STEPS = 4, int(os.environ.get("STEPS", "32"))
BLOCKS = int(os.environ.get("BLOCKS", "512"))
r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=WARM + STEPS)
lib.vspg_w3_timeline_read.argtypes = [C.c_void_p, C.c_int]
buf = np.zeros((BLOCKS, 8, 32), dtype=np.uint64)


def read():
    rc = lib.vspg_w3_timeline_read(buf.ctypes.data, BLOCKS)
    assert rc == 0, rc
    return buf.astype(np.float64)


for w in range(WARM):
    r.render_wave(w, w + 1); r.post_process_wave()
read()
TICK_US = 0.01
rows = []
print("kernel: %s, %d workgroups x 8 wavefronts, tick = 10 ns" % (r.kernel_name(), BLOCKS))
print("%4s %8s %8s %8s %8s %8s %8s %8s | %s" % ("wave", "span_us", "to_exh", "drain", "tail", "ramp", "ideal", "ceiling",
                                                 "per phase (ramp/steady/drain): chunks, mean lanes, us per chunk"))
kinds = []   # per launch: (no parked samples to resolve?, steady-phase us per chunk of each kind [vertex, segment, fresh], steady chunks per kind)
after_update = False
for w in range(WARM, WARM + STEPS):
    r.render_wave(w, w + 1)
    a = read()
    no_parked = after_update          # the update's flush resolved them: this launch's fresh chunks had none to resolve
    after_update = r.isg_update_due(1)
    r.post_process_wave()
    t = a[..., :4]
    ran = t[..., 0] > 0
    assert ran.all(), "a wavefront left no record: BLOCKS does not match the launch"
    t0, t1 = t[..., 0].min(), t[..., 3].max()
    span = (t1 - t0) * TICK_US
    has_exh = t[..., 2] > 0
    to_exh = np.median((t[..., 2] - t[..., 0])[has_exh]) * TICK_US
    drain = np.median((t[..., 3] - t[..., 2])[has_exh]) * TICK_US
    tail = np.median((t1 - t[..., 2])[has_exh]) * TICK_US
    has_full = t[..., 1] > 0
    ramp = np.median((t[..., 1] - t[..., 0])[has_full]) * TICK_US
    s = a[..., 4:31].reshape(BLOCKS, 8, 3, 3, 3).sum(axis=(0, 1))   # [phase][kind][chunks, lanes, ticks]
    steady = s[1]
    # ticks per lane of each kind in the steady phase (chunks are full there), and the share of a wavefront's steady time inside chunks
    per_lane = steady[:, 2] / np.maximum(steady[:, 1], 1)
    steady_span = np.where(has_exh, t[..., 2], t[..., 3]) - np.where(has_full, t[..., 1], t[..., 0])
    in_chunks = steady[:, 2].sum() / steady_span.sum()
    work_ticks = (s[:, :, 1] * per_lane[None, :]).sum()
    ideal = work_ticks / in_chunks / (BLOCKS * 8) * TICK_US
    ph = " / ".join("%d, %.1f, %.2f" % (s[p, :, 0].sum(), s[p, :, 1].sum() / max(1, s[p, :, 0].sum()),
                                        s[p, :, 2].sum() / max(1, s[p, :, 0].sum()) * TICK_US) for p in range(3))
    rows.append((span, to_exh, drain, tail, ramp, ideal, span - ideal, in_chunks))
    kinds.append((no_parked, steady[:, 2] / np.maximum(steady[:, 0], 1) * TICK_US, steady[:, 0], s[0, :, 2] / np.maximum(s[0, :, 0], 1) * TICK_US))
    print("%4d %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f | %s" % (w, span, to_exh, drain, tail, ramp, ideal, span - ideal, ph))
m = np.median(np.array(rows), axis=0)
print("median span %.1f us, to_exh %.1f, drain %.1f, tail %.1f, ramp %.1f, ideal %.1f, ceiling %.1f us = %.1f %% of the span; steady share of time in chunks %.3f"
      % (m[0], m[1], m[2], m[3], m[4], m[5], m[6], 100 * m[6] / m[0], m[7]))
# time per chunk by kind, launches whose fresh chunks resolve a parked sample against those right behind an update (none parked)
for flag, name in ((False, "with parked samples"), (True, "behind an update (none parked)")):
    sel = [k for k in kinds if k[0] == flag]
    if not sel:
        continue
    st = np.median(np.array([k[1] for k in sel]), axis=0)
    rp = np.median(np.array([k[3] for k in sel]), axis=0)
    print("%-32s %2d launches: steady us per chunk vertex %.2f segment %.2f fresh %.2f; ramp phase vertex %.2f segment %.2f fresh %.2f"
          % (name, len(sel), st[0], st[1], st[2], rp[0], rp[1], rp[2]))
    for k in sel if flag else []:
        print("    steady fresh chunks %d at %.2f us, ramp fresh %.2f us" % (k[2][2], k[1][2], k[3][2]))
r.close()
